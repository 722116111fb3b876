#!/usr/bin/env python3
"""MoE encoder (MVMoE), training graph: the sublayer's forward + backward and a whole REINFORCE step, native sparse experts
(train._MoEExpertsFn) against the all-torch expression (train.moe_autograd, EAMRL_MOE_NATIVE_BACKWARD=0), timed on the GPU.

    python tools/time_moe_train.py [--out profiles/rNNx_time_moe_train.json] [--iters 20] [--warmup 3] [--parent-root DIR]

4 experts, top-2, noisy gating, train() mode.  HIP events around each call, `--warmup` untimed calls, then `--iters` timed ones
per path, the two paths alternating in one process; median and [min, max] in ms.  Peak memory: torch.cuda.max_memory_allocated
over one call, as the increase over what was allocated before it (inputs, parameters and packs excluded; the native path's
first call, so that its backward scratch counts), measured before the timing loops, the torch path first.

  (a) sublayer   one MoE(h) forward + backward at 51 712 rows (CVRP-100 x 512) and at 2 560 rows
  (b) step       reinforce_loss(policy, env, td, baseline="no"); loss.backward() of the 3-layer MoE policy on CVRP-100 x 512

--parent-root DIR: a checkout of the parent commit with its own built library.  The same measurement is then repeated by a child
process on that tree (which has the torch expression only) after this process's own, and stored under "parent": the two builds
cannot alternate in one process, so they run back to back in one session.  --root is what the child is started with.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile


def early_root():
    for i, a in enumerate(sys.argv):
        if a == "--root" and i + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[i + 1])
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


ROOT = early_root()
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import eam_rl4co_amd as ea  # noqa: E402
from eam_rl4co_amd import train  # noqa: E402

DEV = "cuda"
MOE = {"encoder": {"hidden_act": "ReLU", "num_experts": 4, "k": 2, "noisy_gating": True}, "decoder": None}
SWITCH = "EAMRL_MOE_NATIVE_BACKWARD"
HAS_NATIVE = hasattr(train, "moe_autograd_native")
PATHS = (("torch", "0"), ("native", "1")) if HAS_NATIVE else (("torch", "0"),)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def peak_increase_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def measure(fns, iters, warmup):
    """fns: {path name: callable}.  -> {name: {time summary, peak_increase_mb}}"""
    out = {n: {"peak_increase_mb": peak_increase_mb(fn)} for n, fn in fns.items()}
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in fns}
    for _ in range(iters):
        for n, fn in fns.items():
            ms[n].append(timed(fn)[0])
    for n in fns:
        out[n].update(summary(ms[n]))
    return out


def with_switch(value, fn):
    def call():
        old = os.environ.get(SWITCH)
        os.environ[SWITCH] = value
        try:
            return fn()
        finally:
            if old is None:
                del os.environ[SWITCH]
            else:
                os.environ[SWITCH] = old
    return call


def sublayer_case(rows, iters, warmup):
    from eam_rl4co_amd.policy import MoE

    torch.manual_seed(rows)
    m = MoE(128, 128, num_neurons=[512], **MOE["encoder"]).train()
    with torch.no_grad():
        m.w_gate.normal_(0, 0.05)          # a trained gate does not tie; the reference's zeros would
        m.w_noise.normal_(0, 0.05)
    m.to(DEV)
    h = torch.randn(rows, 128, device=DEV, requires_grad=True)
    dy = torch.randn(rows, 128, device=DEV)

    def step():
        fn = train.moe_autograd_native if HAS_NATIVE and train.moe_native_backward(m, h) else train.moe_autograd
        y = fn(m, h, True)
        y.backward(dy)
        h.grad = None
        for p in m.parameters():
            p.grad = None

    res = measure({n: with_switch(v, step) for n, v in PATHS}, iters, warmup)
    return {"rows": rows, **{f"sublayer_{n}": r for n, r in res.items()}}


def policy_case(iters, warmup, batch=512, n=100):
    torch.manual_seed(n)
    env = ea.get_env("cvrp", generator_params=dict(num_loc=n))
    td = env.reset(batch_size=[batch]).to(DEV)
    pol = ea.AttentionModelPolicy(env_name="cvrp", moe_kwargs=MOE).train()
    with torch.no_grad():
        for layer in pol.encoder.net.layers:
            layer[2].module.w_gate.normal_(0, 0.05)
            layer[2].module.w_noise.normal_(0, 0.05)
    pol.to(DEV)

    def step():
        out = train.reinforce_loss(pol, env, td.clone(), baseline="no")
        out["loss"].backward()
        for p in pol.parameters():
            p.grad = None

    res = measure({nm: with_switch(v, step) for nm, v in PATHS}, iters, warmup)
    return {"shape": f"cvrp{n}x{batch}", "rows_per_layer": batch * (n + 1), **{f"step_{nm}": r for nm, r in res.items()}}


def ratios(res):
    for case in res["sublayer"] + [res["step"]]:
        keys = [k for k in case if k.endswith("_native")]
        for k in keys:
            t = k.replace("_native", "_torch")
            case["speedup_native_vs_torch"] = case[t]["median_ms"] / case[k]["median_ms"]
            case["ranges_overlap"] = not (case[k]["max_ms"] < case[t]["min_ms"] or case[t]["max_ms"] < case[k]["min_ms"])
            case["peak_ratio_native_vs_torch"] = case[k]["peak_increase_mb"] / case[t]["peak_increase_mb"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--root", default=None, help="the tree to import (default: this file's)")
    ap.add_argument("--parent-root", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_moe_train: no GPU; nothing is measured on a CPU")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "warmup": args.warmup,
           "num_experts": 4, "k": 2, "noisy_gating": True, "native_path_present": HAS_NATIVE,
           "sublayer": [sublayer_case(rows, args.iters, args.warmup) for rows in (51712, 2560)]}
    res["step"] = policy_case(args.iters, args.warmup)
    if HAS_NATIVE:
        ratios(res)
    print(json.dumps(res), flush=True)
    if args.parent_root:
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "parent.json")
            env = {k: v for k, v in os.environ.items() if k not in (SWITCH, "EAMRL_HIP_LIB")}
            subprocess.run([sys.executable, os.path.abspath(__file__), "--root", args.parent_root, "--out", out, "--iters",
                            str(args.iters), "--warmup", str(args.warmup)], check=True, env=env, timeout=900)
            with open(out) as f:
                res["parent"] = json.load(f)
        for mine, theirs in zip(res["sublayer"] + [res["step"]], res["parent"]["sublayer"] + [res["parent"]["step"]]):
            key = "sublayer" if "rows" in mine else "step"
            if f"{key}_native" in mine:
                a, b = mine[f"{key}_native"], theirs[f"{key}_torch"]
                mine["speedup_native_vs_parent"] = b["median_ms"] / a["median_ms"]
                mine["ranges_overlap_with_parent"] = not (a["max_ms"] < b["min_ms"] or b["max_ms"] < a["min_ms"])
                mine["switch_off_vs_parent"] = mine[f"{key}_torch"]["median_ms"] / b["median_ms"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
