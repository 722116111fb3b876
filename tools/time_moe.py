#!/usr/bin/env python3
"""MoE encoder (MVMoE): the feed-forward sublayer's three launches and the rollout around them, timed on the GPU.

    python tools/time_moe.py [--out profiles/rNNx_time_moe.json] [--iters 20] [--warmup 3]

Shapes: CVRP-100 x 1024 (103 424 rows per layer) and TSP-20 x 128 (2 560 rows), 4 experts, top-2, eval mode.  HIP events around
each call, `--warmup` untimed calls, then `--iters` timed ones per path, the paths of a comparison alternating in one process;
median and [min, max] in ms.  The parent commit has no MoE, so no comparison is against an older build:

  (a) sublayer   ops.moe_ffn (memset + gate + grouped expert GEMM + combine) against the same sublayer in PyTorch-ROCm ops under
                 no_grad, in the reference's dispatcher formulation (nonzero / sort / split / per-expert MLP / cat / index_add,
                 with its one host synchronisation for the part sizes); the outputs are compared
  (b) floor      the same call against the plain FFN's two ops.linear launches on the same rows.  Top-2 does twice the dense
                 FFN's arithmetic, so the floor of the ratio is k = 2; the rest is the gate launch, the combine launch and the
                 gather / scatter through the [rows, k, 128] buffer between the 64-row expert groups and the combine (the
                 per-kernel split needs a kernel trace: not taken here)
  (c) rollout    the greedy rollout of the MoE policy against the plain policy on the layer-by-layer encoder
                 (EAMRL_FUSED_ENCODER=0), and, for scale, the plain policy on its default fused encoder
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import eam_rl4co_amd as ea  # noqa: E402
from eam_rl4co_amd import ops  # noqa: E402

DEV = "cuda"
MOE = {"encoder": {"hidden_act": "ReLU", "num_experts": 4, "k": 2, "noisy_gating": True}, "decoder": None}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def alternate(fns, iters, warmup):
    """{name: (summary, last output)} of the callables in `fns`, alternating."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms, outs = {n: [] for n in fns}, {}
    for _ in range(iters):
        for n, fn in fns.items():
            t, outs[n] = timed(fn)
            ms[n].append(t)
    return {n: (summary(v), outs[n]) for n, v in ms.items()}


def dispatcher_sublayer(x, m):
    """h + MoE(h) in torch ops, eval mode, formulated as the reference's SparseDispatcher does it."""
    n = m.num_experts
    p = torch.softmax(x @ m.w_gate, -1)
    top_p, top_i = p.topk(min(m.k + 1, n), dim=-1)
    top_p, top_i = top_p[:, :m.k], top_i[:, :m.k]
    gates = torch.zeros_like(p).scatter(-1, top_i, top_p / (top_p.sum(1, keepdim=True) + 1e-6))
    nz = torch.nonzero(gates)
    order = nz[:, 1].sort(0).indices
    rows, experts = nz[order, 0], nz[order, 1:2]
    sizes = (gates > 0).sum(0).tolist()                     # the host synchronisation of the formulation
    parts = x[rows].split(sizes, 0)
    outs = [F.linear(F.relu(F.linear(part, ex.lins[0].weight, ex.lins[0].bias)), ex.lins[1].weight, ex.lins[1].bias)
            for part, ex in zip(parts, m.experts)]
    stitched = torch.cat(outs, 0) * gates[rows].gather(1, experts)
    return x + torch.zeros_like(x).index_add(0, rows, stitched)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_moe: no GPU; nothing is measured on a CPU")

    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "warmup": args.warmup,
           "num_experts": 4, "k": 2, "cases": []}
    for env_name, n, b in (("tsp", 20, 128), ("cvrp", 100, 1024)):
        torch.manual_seed(n)
        env = ea.get_env(env_name, generator_params=dict(num_loc=n))
        td = env.reset(batch_size=[b]).to(DEV)
        moe_pol = ea.AttentionModelPolicy(env_name=env_name, moe_kwargs=MOE).eval()
        plain = ea.AttentionModelPolicy(env_name=env_name).eval()
        with torch.no_grad():
            for layer in moe_pol.encoder.net.layers:
                layer[2].module.w_gate.normal_(0, 0.05)         # a trained gate does not tie; the reference's zeros would
        moe_pol, plain = moe_pol.to(DEV), plain.to(DEV)
        m = moe_pol.encoder.net.layers[0][2].module
        ffn = plain.encoder.net.layers[0][2].module
        with torch.no_grad():
            h = moe_pol.encoder.init_embedding(td)
            h = h.reshape(-1, 128).contiguous()
        rows = h.shape[0]

        def native():
            with torch.no_grad():
                return m.sublayer(h)

        def torch_ops():
            with torch.no_grad():
                return dispatcher_sublayer(h, m)

        def dense_ffn():
            with torch.no_grad():
                x = ops.linear(h, ffn.lins[0].weight, ffn.lins[0].bias, relu=True)
                return ops.linear(x, ffn.lins[1].weight, ffn.lins[1].bias, residual=h)

        sub = alternate({"native": native, "torch": torch_ops, "dense_ffn": dense_ffn}, args.iters, args.warmup)
        with torch.no_grad():
            _, sel, _ = m.sublayer(h, return_routing=True)
        load = torch.bincount(sel.reshape(-1).long(), minlength=4).tolist()
        diff = float((sub["native"][1] - sub["torch"][1]).abs().max())
        flops = 2 * 2 * 128 * 512 * 2 * rows                        # k experts x two 128 x 512 products per row
        nat, tor, den = (sub[k][0]["median_ms"] for k in ("native", "torch", "dense_ffn"))

        def rollout(pol, fused):
            def call():
                old = os.environ.get("EAMRL_FUSED_ENCODER")
                if not fused:
                    os.environ["EAMRL_FUSED_ENCODER"] = "0"
                try:
                    with torch.no_grad():
                        return pol(td, env, phase="test", decode_type="greedy")
                finally:
                    if not fused:
                        if old is None:
                            del os.environ["EAMRL_FUSED_ENCODER"]
                        else:
                            os.environ["EAMRL_FUSED_ENCODER"] = old
            return call

        ro = alternate({"moe": rollout(moe_pol, True), "plain_layerwise": rollout(plain, False),
                        "plain_fused": rollout(plain, True)}, args.iters, args.warmup)
        case = {
            "shape": f"{env_name}{n}x{b}", "rows": rows, "rows_per_expert": load,
            "sublayer_native": sub["native"][0], "sublayer_torch_dispatcher": sub["torch"][0], "dense_ffn_two_linears": sub["dense_ffn"][0],
            "a_speedup_native_vs_torch": tor / nat,
            "a_max_abs_difference_native_vs_torch": diff,
            "b_ratio_native_vs_dense_ffn": nat / den, "b_floor": 2.0,
            "expert_gflop": flops / 1e9, "native_tflops_of_expert_arithmetic": flops / (nat * 1e-3) / 1e12,
            "rollout_moe": ro["moe"][0], "rollout_plain_layerwise": ro["plain_layerwise"][0], "rollout_plain_fused": ro["plain_fused"][0],
            "c_ratio_moe_vs_plain_layerwise": ro["moe"][0]["median_ms"] / ro["plain_layerwise"][0]["median_ms"],
            "reward_mean_moe": float(ro["moe"][1]["reward"].mean()), "reward_mean_plain": float(ro["plain_layerwise"][1]["reward"].mean()),
        }
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
