"""The evolutionary improvement step (EA.run) on graphs beyond the LDS kernel, next to the other stages of an EAM step.

    python tools/time_ea_large.py [--rounds 3] [--reps 3] [--shapes tsp200,tsp500,cvrp200,cvrp500] [--skip-stages]
                                  [--parent-lib path/to/libeamrl_hip.so] [--json out.json]

Per shape (env, nodes, instances B, starts S), G = 3 generations, the reference's default rates 0.1 / 0.6 / 0.2:
  ea_ms ........ `EA.run` on the sampled tours (the device-memory path: 2 + 5 G launches), HIP events around the call;
  rollout_ms ... the sampled multistart rollout of the same batch, `policy(td, env, phase="train", num_starts=S)` without grad;
  reeval_ms .... the native teacher-forced re-evaluation of the same tours with its backward,
                 `policy(..., actions=tours)` + `log_likelihood.sum().backward()`.
Every figure is the median over `rounds` rounds of the median over `reps` calls, after a warm-up of each; the rounds are kept.
The reference's numba operators cannot run next to these: numba is absent here (tests/golden/_refshim.py runs them as plain
Python for the goldens), so there is no reference time.

--parent-lib: the regression guard for the LDS kernel.  `eamrl_ea_tsp_run` / `eamrl_ea_cvrp_run` of this tree's library and
of another build of the library (the parent commit's) on the same 64 x 100 x 100 populations and draws, alternating, three
rounds in one process; both series are recorded and the tree must lie inside the parent's own run-to-run spread.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import eam_rl4co_amd as ea  # noqa: E402
from eam_rl4co_amd import _lib, ops  # noqa: E402

DEV = "cuda"
SHAPES = {"tsp200": ("tsp", 200, 64, 200), "tsp500": ("tsp", 500, 16, 500), "cvrp200": ("cvrp", 200, 64, 200),
          "cvrp500": ("cvrp", 500, 16, 100)}
G, RATES = 3, dict(mutation_rate=0.1, crossover_rate=0.6, selection_rate=0.2)


def event_ms(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def rounds_of(fn, rounds, reps, warmup=2):
    for _ in range(warmup):
        fn()
    series = [statistics.median(event_ms(fn)[0] for _ in range(reps)) for _ in range(rounds)]
    return {"ms": round(statistics.median(series), 4), "ms_rounds": [round(x, 4) for x in series]}


def policy_for(env_name):
    kw = dict(num_encoder_layers=6, normalization="instance", use_graph_context=False) if env_name == "tsp" else {}
    return ea.AttentionModelPolicy(env_name=env_name, **kw).to(DEV)


def time_shape(name, args):
    env_name, N, B, S = SHAPES[name]
    torch.manual_seed(11)
    env = ea.get_env(env_name, generator_params=dict(num_loc=N), seed=11)
    td = env.reset(batch_size=[B]).to(DEV)
    pol = policy_for(env_name)
    with torch.no_grad():
        out = pol(td.clone(), env, phase="train", decode_type="multistart_sampling", num_starts=S)
    pop = ea.unbatchify(out["actions"], S).contiguous()
    L = pop.shape[-1]
    runner = ea.EA(env, dict(num_generations=G, **RATES))
    gen = torch.Generator(device=DEV).manual_seed(3)
    draws = (ea.EADraws.sample(G, B, S, N, RATES["selection_rate"], DEV, gen) if env_name == "tsp" else
             ea.EACvrpDraws.sample(G, B, S, RATES["selection_rate"], DEV, gen))
    res = {"env": env_name, "num_loc": N, "instances": B, "starts": S, "row_length": L, "generations": G,
           "pairs_per_instance": ops.ea_num_pairs(RATES["selection_rate"], S), "kernel": ops.ea_kernel(env_name, S, N, L)}
    res["ea"] = rounds_of(lambda: runner.run(pop, td, draws=draws), args.rounds, args.reps)
    new_pop, fit = runner.run(pop, td, draws=draws)
    res["tours_changed"] = int((new_pop != pop).any(-1).sum())
    if not args.skip_stages:
        def rollout():
            with torch.no_grad():
                return pol(td.clone(), env, phase="train", decode_type="multistart_sampling", num_starts=S)

        def reeval():
            for p in pol.parameters():
                p.grad = None
            o = pol(td.clone(), env, phase="train", num_starts=S, actions=out["actions"])
            o["log_likelihood"].sum().backward()

        res["rollout"] = rounds_of(rollout, args.rounds, args.reps, warmup=1)
        res["reeval_fwd_bwd"] = rounds_of(reeval, args.rounds, args.reps, warmup=1)
        total = res["ea"]["ms"] + res["rollout"]["ms"] + res["reeval_fwd_bwd"]["ms"]
        res["ea_share_of_rollout_ea_reeval"] = round(res["ea"]["ms"] / total, 4)
    return res


def lds_guard(parent_path, rounds=3, reps=10):
    """Tree and parent builds of the LDS entry points on the same inputs, alternating."""
    libs = {"tree": _lib.load(), "parent": C.CDLL(parent_path)}
    for fn in ("eamrl_ea_tsp_run", "eamrl_ea_cvrp_run"):
        getattr(libs["parent"], fn).argtypes = _lib.PROTOTYPES[fn]
        getattr(libs["parent"], fn).restype = C.c_int
    B, S, N = 64, 100, 100
    P = ops.ea_num_pairs(RATES["selection_rate"], S)
    ptr, stream = ops._ptr, lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"what": f"LDS kernel k_ea, {B} instances x {S} tours x {N} nodes, G = {G}, default rates; tree and parent builds of "
                   f"the library alternating in one process, {rounds} rounds of the median over {reps} calls (HIP events)"}
    for env_name in ("tsp", "cvrp"):
        torch.manual_seed(5)
        env = ea.get_env(env_name, generator_params=dict(num_loc=N), seed=5)
        td = env.reset(batch_size=[B]).to(DEV)
        with torch.no_grad():
            acts = policy_for(env_name)(td.clone(), env, phase="train", decode_type="multistart_sampling", num_starts=S)["actions"]
        pop0 = ea.unbatchify(acts, S).contiguous()
        L = pop0.shape[-1]
        assert ops.ea_kernel(env_name, S, N, L) == "lds"
        gen = torch.Generator(device=DEV).manual_seed(3)
        fit = torch.empty(B, S, device=DEV)
        locs = td["locs"].contiguous()
        if env_name == "tsp":
            d = ea.EADraws.sample(G, B, S, N, RATES["selection_rate"], DEV, gen)
            tail = (ptr(d.cross_rand), ptr(d.cross_idx), ptr(d.mut_rand), ptr(d.mut_idx))

            def call(lib, pop):
                return lib.eamrl_ea_tsp_run(ptr(locs), ptr(pop), ptr(fit), B, S, N, G, 0.1, float(np.float32(0.6)), 0.2,
                                            *tail, stream())
        else:
            d = ea.EACvrpDraws.sample(G, B, S, RATES["selection_rate"], DEV, gen)
            dem, vcap = td["demand"].contiguous(), td["vehicle_capacity"].reshape(B).float().contiguous()
            tail = (ptr(d.init_mut_rand), ptr(d.init_mut_u), ptr(d.cross_rand), ptr(d.cross_u), ptr(d.mut_rand), ptr(d.mut_u))

            def call(lib, pop):
                return lib.eamrl_ea_cvrp_run(ptr(locs), ptr(dem), ptr(vcap), ptr(pop), ptr(fit), B, S, N, L, G, 0.1, 0.6, 0.2, 0,
                                             *tail, stream())
        results, series = {}, {"tree": [], "parent": []}
        for which, lib in libs.items():                    # warm-up, and the two builds must agree
            for _ in range(3):
                pop = pop0.clone()
                assert call(lib, pop) == 0
            torch.cuda.synchronize()
            results[which] = (pop.clone(), fit.clone())
        assert torch.equal(results["tree"][0], results["parent"][0]) and torch.equal(results["tree"][1], results["parent"][1])
        for _ in range(rounds):
            for which in ("parent", "tree"):
                ms = []
                for _ in range(reps):
                    pop = pop0.clone()
                    ms.append(event_ms(lambda: call(libs[which], pop))[0])
                series[which].append(round(statistics.median(ms), 4))
        lo, hi = min(series["parent"]), max(series["parent"])
        out[env_name] = {"row_length": L, "pairs_per_instance": P, "parent_ms_rounds": series["parent"],
                         "tree_ms_rounds": series["tree"], "parent_spread_ms": [lo, hi],
                         "tree_median_inside_parent_spread": bool(lo <= statistics.median(series["tree"]) <= hi),
                         "tree_over_parent": round(statistics.median(series["tree"]) / statistics.median(series["parent"]), 4),
                         "results_identical": True}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--skip-stages", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU timing"
    out = {"what": "EA.run (G = 3, rates 0.1 / 0.6 / 0.2) on the device-memory path next to the sampled multistart rollout and the "
                   "native re-evaluation (forward + backward) of the same batch; one MI355X, fp32, untrained policy; median over "
                   f"{args.rounds} rounds of the median over {args.reps} calls, HIP events",
           "reference": "not timed: the reference's operators need numba, which is absent here",
           "shapes": {}}
    for name in [s for s in args.shapes.split(",") if s]:
        out["shapes"][name] = time_shape(name, args)
        print(json.dumps({name: out["shapes"][name]}), flush=True)
    if args.parent_lib:
        out["lds_guard"] = lds_guard(args.parent_lib)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
