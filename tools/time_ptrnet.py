#!/usr/bin/env python3
"""Pointer Network rollout: the native path against the policy's own PyTorch expression on the same GPU.

    python tools/time_ptrnet.py [--out profiles/rNNx_time_ptrnet.json] [--iters 20] [--warmup 3]

Shapes: TSP-20 x 128 and TSP-100 x 1024, greedy and seeded sampling.  HIP events around the policy call, `--warmup` untimed
calls, then `--iters` timed ones per path, the two paths alternating in one process; median and [min, max] in ms.  The parent
commit has no Pointer Network, so the baseline is `PointerNetworkPolicy.torch_rollout` under no_grad (the same model in
PyTorch-ROCm ops, N steps of a dozen launches each), not an older build of the code under test.  At every timed size the tours
of the two paths are compared on the rows whose float64 decision margin (tests/ptrnet_ref.py) is at least 1e-4.
The step's arithmetic: 2 N 128 tanh and two 128 x 512 products (plus two 128 x 128) per instance and step."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import eam_rl4co_amd as ea  # noqa: E402
import ptrnet_ref  # noqa: E402

DEV = "cuda"
MIN_GAP = 1e-4


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    pol = ea.PointerNetworkPolicy()
    shapes = {k: tuple(v.shape) for k, v in pol.state_dict().items()}
    pol.load_state_dict(ptrnet_ref.closed_form_weights(shapes))
    pol = pol.to(DEV).eval()
    w64 = {k: v.to(DEV) for k, v in ptrnet_ref.closed_form_weights(shapes, torch.float64).items()}
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "warmup": args.warmup,
           "baseline": "PointerNetworkPolicy.torch_rollout under no_grad (PyTorch-ROCm ops on the same GPU)", "cases": []}
    for n, b in ((20, 128), (100, 1024)):
        env = ea.TSPEnv(generator_params=dict(num_loc=n))
        torch.manual_seed(n)
        td = env.reset(batch_size=[b]).to(DEV)
        locs = td["locs"].float().contiguous()
        for mode in ("greedy", "sampling"):
            seed = 4321 + n
            noise = ea.ops.exp1_noise(seed, b, n, n, device=DEV) if mode == "sampling" else None

            def native():
                with torch.no_grad():
                    return pol(td, env, phase="test", decode_type=mode, seed=seed if mode == "sampling" else None)

            def baseline():
                with torch.no_grad():
                    acts, lp = pol.torch_rollout(locs, mode, noise=noise)
                    return {"actions": acts, "log_likelihood": lp.sum(1), "reward": ea.ops.tour_length_reward(locs, acts, False)}

            for _ in range(args.warmup):
                native(), baseline()
            torch.cuda.synchronize()
            t_nat, t_base = [], []
            for _ in range(args.iters):
                ms, out_n = timed(native)
                t_nat.append(ms)
                ms, out_b = timed(baseline)
                t_base.append(ms)
            ref_a, _, gap = ptrnet_ref.rollout(w64, locs, mode, noise=noise)
            keep = gap >= MIN_GAP
            case = {
                "shape": f"tsp{n}x{b}", "decode_type": mode, "native": summary(t_nat), "torch": summary(t_base),
                "speedup_median": statistics.median(t_base) / statistics.median(t_nat),
                "rows_compared": int(keep.sum()), "rows": b,
                "tours_equal_native_vs_torch": bool(torch.equal(out_n["actions"][keep], out_b["actions"][keep])),
                "tours_equal_native_vs_float64": bool(torch.equal(out_n["actions"][keep], ref_a[keep])),
                "reward_mean_native": float(out_n["reward"].mean()), "reward_mean_torch": float(out_b["reward"].mean()),
                # per instance-step: 2 N 128 tanh; products 2 * (128 x 512 + 2 * 128 x 128) multiply-adds
                "tanh_per_rollout": 2 * n * 128 * n * b,
                "native_ns_per_tanh": statistics.median(t_nat) * 1e6 / (2 * n * 128 * n * b),
                "native_us_per_step": statistics.median(t_nat) * 1e3 / n,
            }
            print(json.dumps(case), flush=True)
            res["cases"].append(case)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
