"""PolyNet against the Attention Model on the start-sharing rollout kernel, same build, one process, timed alternately.

    python tools/time_polynet_vs_am.py [--batch 256] [--num-loc 100] [--starts 128] [--rounds 5] [--reps 5] [--json out.json]

decode   `ops.rollout` alone (the decode loop: one launch, plus the depot padding launch of CVRP) on a cache and a state built
         before the clock starts, seeded sampling, HIP events.  PolyNetPolicy(k = starts) against AttentionModelPolicy with the
         same encoder settings, both with `starts` rows per instance and no forced start (num_samples).
whole    `policy(td, env, phase="test", decode_type="sampling", num_samples=starts)`: encoder + cache + decode loop + reward, host
         clock around a device synchronise.
Every round takes the median over `reps` calls of each variant in turn; the median over the rounds is reported with [min, max] of
the rounds.  With EAMRL_HIP_LIB pointing at the instrumented build of tools/build_stamps.sh, --stamps adds the PolyNet kernel's
cycles per phase (all wavefronts): which share goes to the poly MFMA phases (waits for the streamed weights included) and to
their three barriers.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import eam_rl4co_amd as ea  # noqa: E402
from eam_rl4co_amd import _lib, ops  # noqa: E402
from eam_rl4co_amd.policy import state_from_td  # noqa: E402

DEV = "cuda"
PHASES = ["q tile build", "barrier", "scores mfma + mask + max", "softmax exps", "value mfma + store", "barrier", "logit mfma",
          "noise", "tanh / mask / tile max", "barrier", "exp + tile sum", "-", "lse + selection", "-", "env transition", "-", "-",
          "poly: g = heads Wout (+ wait for Wout)", "poly: barrier g", "poly: h = relu(W1 g + c)", "poly: barrier h",
          "poly: y = g + W2 h + b2", "poly: barrier y"]


def summary(v):
    return {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def alternate(variants, rounds, reps):
    """{name: fn -> ms} -> {name: summary}; every round visits the variants in turn."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            res[k].append(statistics.median(fn() for _ in range(reps)))
    return {k: summary(v) for k, v in res.items()}


def decode_timer(pol, env, td, S):
    env_name = pol.env_name
    with torch.no_grad():
        hidden, _ = pol.encoder(td)
        cache = pol.decoder._precompute_cache(hidden, num_starts=S)
    M = td["action_mask"].shape[-1]
    t_max = ea.env_spec.max_steps(env_name, M)

    def run():
        st = state_from_td(env_name, td, S)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.rollout(st, cache, "sampling", seed=1234, t_max=t_max, poly=pol._pointer_operands())
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    return run


def whole_timer(pol, env, td, S):
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            pol(td, env, phase="test", decode_type="sampling", num_samples=S)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--num-loc", type=int, default=100)
    ap.add_argument("--starts", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stamps", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU timing"
    B, N, S = args.batch, args.num_loc, args.starts
    out = {"what": f"sampling rollout, {B} instances x {S} rows, one MI355X, fp32, untrained policies; {args.rounds} rounds (variants "
                   f"alternating) of the median over {args.reps} calls; ms = median of the rounds, with their min and max"}
    for env_name in ("tsp", "cvrp"):
        torch.manual_seed(7)
        env = ea.get_env(env_name, generator_params=dict(num_loc=N), seed=7)
        td = env.reset(batch_size=[B]).to(DEV)
        poly = ea.PolyNetPolicy(k=S, env_name=env_name).eval().to(DEV)
        am = ea.AttentionModelPolicy(env_name=env_name, num_encoder_layers=6, normalization="instance").eval().to(DEV)
        r = {"decode_ms": alternate({"polynet": decode_timer(poly, env, td, S), "am": decode_timer(am, env, td, S)},
                                    args.rounds, args.reps),
             "whole_ms": alternate({"polynet": whole_timer(poly, env, td, S), "am": whole_timer(am, env, td, S)},
                                   args.rounds, args.reps)}
        r["polynet_over_am_decode"] = round(r["decode_ms"]["polynet"]["ms"] / r["decode_ms"]["am"]["ms"], 3)
        r["polynet_over_am_whole"] = round(r["whole_ms"]["polynet"]["ms"] / r["whole_ms"]["am"]["ms"], 3)
        if args.stamps:
            lib = _lib.load()
            buf = (C.c_ulonglong * 24)()
            fn = decode_timer(poly, env, td, S)
            lib.eamrl_debug_read_ms_stamps(buf, 1)
            fn()
            lib.eamrl_debug_read_ms_stamps(buf, 0)
            tot = sum(buf[i] for i in range(23) if i != 16)
            r["polynet_phase_share"] = {f"{i:02d} {PHASES[i]}": round(buf[i] / tot, 4) for i in range(23) if i != 16 and buf[i]}
        out[f"{env_name}{N}"] = r
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
