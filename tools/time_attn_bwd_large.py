"""Encoder self-attention backward above 112 nodes: the native kernel (k_mha_encoder_bwd_mfma) against torch's
scaled_dot_product_attention, timed alternately in one process, with the peak device memory of each.

    python tools/time_attn_bwd_large.py [--iters 20] [--steps 3] [--no-train] [--json out.json]

Rows:
  attn   one layer's attention at CVRP-500 x 64, TSP-200 x 256 and CVRP-1000 x 16 (random packed qkv): the backward alone
         (native: ops.mha_encoder_backward; torch: autograd.grad through SDPA on the permuted [B, H, N, D] views, as
         train._self_attention builds them), and forward + backward with the peak of torch.cuda.max_memory_allocated over it;
  train  a whole train.reinforce_loss + backward at CVRP-500 x 64 for an instance-norm and a batch-norm policy, native against
         EAMRL_TORCH_ATTENTION=1 (torch's attention in the graph; instance norm then also takes two encoder passes).
Every round runs each path once, in alternating order; medians are reported.  Run under `rocprofv3 --kernel-trace --stats`
(with --no-train --iters 5) for the kernel times and the SDPA backend torch picks.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

import eam_rl4co_amd as ea  # noqa: E402
from eam_rl4co_amd import ops, train  # noqa: E402

SHAPES = [("cvrp500x64", 64, 501), ("tsp200x256", 256, 200), ("cvrp1000x16", 16, 1001)]
E, H, D = 128, 8, 16


def sdpa(qkv, B, N):
    q = qkv.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    return F.scaled_dot_product_attention(q[0], q[1], q[2]).permute(0, 2, 1, 3).reshape(B, N, E)


def timed(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def attn_rows(iters):
    rows = []
    for name, B, N in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(N)
        qkv = (torch.randn(B, N, 3 * E, generator=g) * 1.5).cuda()
        dout = torch.randn(B, N, E, generator=g).cuda()
        qg = qkv.clone().requires_grad_()
        y = sdpa(qg, B, N)

        def nat_bwd():
            ops.mha_encoder_backward(qkv, dout, H)

        def tor_bwd():
            torch.autograd.grad(y, qg, dout, retain_graph=True)

        def nat_fb():
            q = qkv.clone().requires_grad_()
            train._self_attention(q, B, N, E, H).backward(dout)

        def tor_fb():
            q = qkv.clone().requires_grad_()
            sdpa(q, B, N).backward(dout)

        for f in (nat_bwd, tor_bwd, nat_fb, tor_fb):
            f()
        t = {k: [] for k in ("native_bwd", "torch_bwd", "native_fwd_bwd", "torch_fwd_bwd")}
        for i in range(iters):
            pairs = [("native_bwd", nat_bwd), ("torch_bwd", tor_bwd)]
            pairs += [("native_fwd_bwd", nat_fb), ("torch_fwd_bwd", tor_fb)]
            if i % 2:
                pairs = pairs[1::-1] + pairs[:1:-1]
            for k, f in pairs:
                t[k].append(timed(f))
        row = dict(row="attn", shape=name, B=B, N=N, **{k + "_ms": statistics.median(v) for k, v in t.items()})
        del y
        row["native_peak_mb"] = peak_mb(nat_fb)
        row["torch_peak_mb"] = peak_mb(tor_fb)
        # the kernel's own work: S and dP (2 x 2 N^2 D), dV, dK, dq (3 x 2 N^2 D) per (instance, head)
        row["native_bwd_tflops"] = 10 * N * N * D * B * H / (row["native_bwd_ms"] * 1e-3) / 1e12
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def train_rows(steps):
    rows = []
    env = ea.get_env("cvrp", generator_params=dict(num_loc=500), seed=1)
    torch.manual_seed(1)
    td = env.reset(batch_size=[64]).cuda()
    for norm in ("instance", "batch"):
        torch.manual_seed(0)
        pol = ea.AttentionModelPolicy(env_name="cvrp", normalization=norm).cuda().train()

        def step():
            for p in pol.parameters():
                p.grad = None
            out = train.reinforce_loss(pol, env, td.clone(), baseline="mean")
            out["loss"].backward()

        t = {"native": [], "torch": []}
        peak = {}
        for i in range(steps + 1):
            order = ("native", "torch") if i % 2 == 0 else ("torch", "native")
            for which in order:
                os.environ["EAMRL_TORCH_ATTENTION"] = "1" if which == "torch" else "0"
                if i == 0:      # warm-up, and the peak memory of one step
                    peak[which] = peak_mb(step)
                else:
                    t[which].append(timed(step))
        os.environ.pop("EAMRL_TORCH_ATTENTION", None)
        row = dict(row="train", shape="cvrp500x64", norm=norm, native_step_ms=statistics.median(t["native"]),
                   torch_step_ms=statistics.median(t["torch"]), native_peak_mb=peak["native"], torch_peak_mb=peak["torch"],
                   steps=steps)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to time")
    rows = attn_rows(a.iters)
    if not a.no_train:
        rows += train_rows(a.steps)
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__,
               sdpa_flags=dict(flash=torch.backends.cuda.flash_sdp_enabled(), mem_efficient=torch.backends.cuda.mem_efficient_sdp_enabled(),
                               math=torch.backends.cuda.math_sdp_enabled()),
               rows=rows)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
