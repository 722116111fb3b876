"""PDP-100 against CVRP-100 greedy rollouts on the same build, timed alternately in one process.

    python tools/time_pdp_vs_cvrp.py [--batch 1024] [--num-loc 100] [--rounds 5] [--reps 10] [--json out.json]

whole  = `policy(td, env, phase="test", decode_type="greedy")`: encoder + cache + decode loop + reward (env.reset excluded),
         host clock around a device synchronise;
decode = the whole-rollout kernel alone (`ops.rollout` on a prebuilt cache), HIP events, and per decode step (CVRP's step
         count depends on the tours; PDP always takes num_loc steps).
Every round takes the median over `reps` rollouts of each env, PDP first, then CVRP; the median over the rounds is reported
together with the rounds themselves (their spread is the run-to-run noise a ratio has to be read against).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import eam_rl4co_amd as ea  # noqa: E402
from eam_rl4co_amd import ops  # noqa: E402
from eam_rl4co_amd.policy import state_from_td  # noqa: E402

DEV = "cuda"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--num-loc", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU timing"
    B, N = args.batch, args.num_loc
    setups = {}
    for env_name in ("pdp", "cvrp"):
        torch.manual_seed(7)
        env = ea.get_env(env_name, generator_params=dict(num_loc=N), seed=7)
        pol = ea.AttentionModelPolicy(env_name=env_name).eval().to(DEV)
        td = env.reset(batch_size=[B]).to(DEV)
        with torch.no_grad():
            hidden, _ = pol.encoder(td)
            cache = pol.decoder._precompute_cache(hidden)
        setups[env_name] = (env, pol, td, cache)

    def whole(env_name):
        env, pol, td, _ = setups[env_name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pol(td, env, phase="test", decode_type="greedy")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def decode(env_name):
        _, _, td, cache = setups[env_name]
        st = state_from_td(env_name, td)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, _, info = ops.rollout(st, cache, "greedy", t_max=(N if env_name == "pdp" else None))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), int(info[0])

    res = {k: {"whole_ms": [], "decode_ms": [], "steps": None} for k in setups}
    with torch.no_grad():
        for k in setups:                      # warm-up of every shape the timed window uses
            for _ in range(5):
                whole(k)
                decode(k)
        for _ in range(args.rounds):
            for k in ("pdp", "cvrp"):
                w = [whole(k)[0] for _ in range(args.reps)]
                d = [decode(k) for _ in range(args.reps)]
                res[k]["whole_ms"].append(statistics.median(w))
                res[k]["decode_ms"].append(statistics.median(x[0] for x in d))
                res[k]["steps"] = d[0][1]
        out = {"what": f"AttentionModel greedy rollout, {B} instances x {N} locations, one MI355X, fp32, untrained policy, eager "
                       f"policy call; {args.rounds} rounds (pdp, cvrp alternating) of the median over {args.reps} rollouts",
               "per_env": {}}
        for k, v in res.items():
            cache = setups[k][3]
            wm, dm = statistics.median(v["whole_ms"]), statistics.median(v["decode_ms"])
            out["per_env"][k] = {
                "whole_ms_rounds": [round(x, 4) for x in v["whole_ms"]], "decode_ms_rounds": [round(x, 4) for x in v["decode_ms"]],
                "whole_ms": round(wm, 4), "decode_ms": round(dm, 4), "decode_steps": v["steps"],
                "decode_us_per_step": round(1e3 * dm / v["steps"], 4), "kernel": ops.rollout_kernel(k, cache, B, v["steps"]),
                "decode_ms_spread": round(max(v["decode_ms"]) - min(v["decode_ms"]), 4),
                "reward_mean": round(float(whole(k)[1]["reward"].mean()), 4)}
    p, c = out["per_env"]["pdp"], out["per_env"]["cvrp"]
    out["pdp_over_cvrp_per_decode_step"] = round(p["decode_us_per_step"] / c["decode_us_per_step"], 4)
    out["cvrp_decode_spread_rel"] = round(c["decode_ms_spread"] / c["decode_ms"], 4)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
