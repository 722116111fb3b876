"""Two builds of the library timed alternately in ONE process on the per-row reward / log-likelihood / validity kernels
(A/B yardstick for changes to env_reward.hip, pdp.hip and tour_row.hpp), in the manner of tools/bench_enc_ab.py.

    bash tools/build_variant.sh parent           # in a checkout of the parent commit; copy the library over
    python tools/time_epilogue.py --a tools/_variants/parent/libeamrl_hip.so --b eam_rl4co_amd/lib/libeamrl_hip.so \
        [--rounds 7] [--window 0.3] [--rows 102400] [--ea] [--json out.json]

Rows, on seeded VALID tours of 100-node graphs (1024 instances, row r belongs to instance r % 1024): eamrl_rollout_finish with
reward + log-likelihood + verdict (TSP at 1024 and `rows` rows, CVRP on depot-padded tours), eamrl_check_solution (tsp, cvrp,
pctsp, pdp), eamrl_op_check_solution, eamrl_tour_length with and without the depot, eamrl_pctsp_reward, eamrl_op_reward.
--ea adds EA.run (the fitness sums of evolution_common.hpp): the shapes of `tools/kernel_bench.py ea` and two device-memory
shapes.  The entry points are called directly on preallocated outputs, so that a window holds launches and little else.
Every round times each build once (device events around as many launches as fill `window` seconds), in alternating order.
Per build: mean, min, max over the rounds; the outputs of the two builds are compared bit for bit.  A row passes when b's
mean is not above a's mean by more than a's own spread (max - min) over the same rounds.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import eam_rl4co_amd as ea  # noqa: E402
from eam_rl4co_amd import _lib, ops  # noqa: E402
from bench_enc_ab import load_lib  # noqa: E402

DEV = "cuda"
B, N = 1024, 100


def window_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def ab_row(name, call, libs, rounds, window, prep=None):
    """call(lib) enqueues the work once and returns the tensors it wrote; prep() resets what a call adds to."""
    outs = {}
    for k, lib in libs.items():
        for _ in range(3):      # warm-up: code objects, kernel attributes, clocks
            call(lib)
        if prep:
            prep()
        got = call(lib)
        torch.cuda.synchronize()
        outs[k] = [t.clone() for t in got]
    once = window_ms(lambda: call(libs["a"]), 10)
    iters = max(3, min(200000, int(window * 1e3 / max(once, 1e-4))))
    samples = {"a": [], "b": []}
    for r in range(rounds):
        for k in (("a", "b") if r % 2 == 0 else ("b", "a")):
            samples[k].append(window_ms(lambda: call(libs[k]), iters))
    same = all(x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(outs["a"], outs["b"]))
    row = {"bit_identical": bool(same), "launches_per_window": iters}
    for k, v in samples.items():
        row[k] = {"mean_ms": round(statistics.mean(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5),
                  "rounds_ms": [round(x, 5) for x in v]}
    spread = row["a"]["max_ms"] - row["a"]["min_ms"]
    row["a_spread_ms"] = round(spread, 5)
    row["b_over_a"] = round(row["b"]["mean_ms"] / row["a"]["mean_ms"], 4)
    row["pass"] = bool(same and row["b"]["mean_ms"] <= row["a"]["mean_ms"] + spread)
    print(json.dumps({name: row}), flush=True)
    return row, outs["a"]


def perms(R, n, gen):
    return torch.rand(R, n, device=DEV, generator=gen).argsort(1)


def cvrp_tours(dem_int, cap, R, gen):
    """Random customer orders cut into routes that fit `cap`, ending on the depot and depot-padded to the longest row."""
    order = perms(R, N, gen)
    d = dem_int[torch.arange(R, device=DEV) % B].gather(1, order)
    ptr = torch.zeros(R, dtype=torch.int64, device=DEV)
    load = torch.zeros(R, dtype=torch.int64, device=DEV)
    cols = []
    while bool((ptr < N).any()):
        at = ptr.clamp(max=N - 1)[:, None]
        nxt = d.gather(1, at)[:, 0]
        can = (ptr < N) & (load + nxt <= cap)
        cols.append(torch.where(can, order.gather(1, at)[:, 0] + 1, torch.zeros_like(ptr)))
        load = torch.where(can, load + nxt, torch.zeros_like(load))
        ptr = ptr + can
    cols.append(torch.zeros_like(ptr))
    return torch.stack(cols, 1).contiguous()


def pdp_tours(R, gen):
    """Random orders of 1..N in which every pickup i stands before its delivery i + N/2."""
    half = N // 2
    pos = perms(R, N, gen)                                  # pos[r, v - 1] = position of node v
    p, d = pos[:, :half], pos[:, half:]
    first, second = torch.minimum(p, d), torch.maximum(p, d)
    tour = torch.empty(R, N, dtype=torch.int64, device=DEV)
    ids = torch.arange(1, half + 1, device=DEV).expand(R, half)
    tour.scatter_(1, first, ids)
    tour.scatter_(1, second, ids + half)
    return tour


def epilogue_rows(libs, args):
    gen = torch.Generator(device=DEV).manual_seed(7)
    R, M = args.rows, N + 1
    ptr = ops._ptr
    stream = torch.cuda.current_stream().cuda_stream
    u = lambda *shape: torch.rand(*shape, device=DEV, generator=gen)      # noqa: E731
    reward, ll = torch.empty(R, device=DEV), torch.empty(R, device=DEV)
    bad = torch.zeros(2, dtype=torch.int32, device=DEV)
    rows = {}

    def add(name, fn, written, valid=True):
        def call(lib):
            rc = fn(lib)
            assert rc == 0, (name, rc)
            return written
        rows[name], got = ab_row(name, call, libs, args.rounds, args.window, prep=bad.zero_)
        if valid and any(t is bad for t in written):
            assert got[-1].tolist() == [0, 0], (name, "the timed tours must be valid", got[-1].tolist())

    # ---- TSP-100 -------------------------------------------------------------------------------------------------------
    locs_t = u(B, N, 2)
    act_t = perms(R, N, gen)
    logp_t = -u(R, N)
    for rr in (1024, R):
        add(f"rollout_finish_tsp100_R{rr}",
            lambda lib, rr=rr: lib.eamrl_rollout_finish(ops.ENV_TSP, ptr(locs_t), ptr(act_t), ptr(logp_t), N, None, None, ptr(reward),
                                                        ptr(ll), ptr(bad), rr, B, N, N, stream), [reward, ll, bad])
    add("check_solution_tsp", lambda lib: lib.eamrl_check_solution(ops.ENV_TSP, ptr(act_t), None, None, R, R, N, N, ptr(bad), stream),
        [bad])
    add("tour_length_tsp", lambda lib: lib.eamrl_tour_length(ptr(locs_t), ptr(act_t), ptr(reward), R, B, N, N, 0, stream), [reward])
    # ---- CVRP-100: depot-padded tours ----------------------------------------------------------------------------------
    locs_d = u(B, M, 2)
    dem_int = torch.randint(1, 10, (B, N), device=DEV, generator=gen)
    demand = (dem_int.float() / 50.0).contiguous()
    vcap = torch.ones(R, device=DEV)
    act_c = cvrp_tours(dem_int, 50, R, gen)
    Tc = act_c.shape[1]
    logp_c = -u(R, Tc)
    add(f"rollout_finish_cvrp100_T{Tc}",
        lambda lib: lib.eamrl_rollout_finish(ops.ENVS["cvrp"], ptr(locs_d), ptr(act_c), ptr(logp_c), Tc, ptr(demand), ptr(vcap),
                                             ptr(reward), ptr(ll), ptr(bad), R, B, M, Tc, stream), [reward, ll, bad])
    add("check_solution_cvrp", lambda lib: lib.eamrl_check_solution(ops.ENVS["cvrp"], ptr(act_c), ptr(demand), ptr(vcap), R, B, N, Tc,
                                                                    ptr(bad), stream), [bad])
    add("tour_length_depot", lambda lib: lib.eamrl_tour_length(ptr(locs_d), ptr(act_c), ptr(reward), R, B, M, Tc, 1, stream), [reward])
    # ---- PCTSP-100: every customer, then the depot -----------------------------------------------------------------------
    act_p = torch.cat([perms(R, N, gen) + 1, torch.zeros(R, 1, dtype=torch.int64, device=DEV)], 1).contiguous()
    prize = torch.cat([torch.zeros(B, 1, device=DEV), u(B, N) * 0.08], 1).contiguous()
    penalty = torch.cat([torch.zeros(B, 1, device=DEV), u(B, N) * 0.12], 1).contiguous()
    add("check_solution_pctsp", lambda lib: lib.eamrl_check_solution(ops.ENVS["pctsp"], ptr(act_p), ptr(prize), None, R, B, N, N + 1,
                                                                     ptr(bad), stream), [bad])
    add("pctsp_reward", lambda lib: lib.eamrl_pctsp_reward(ptr(locs_d), ptr(penalty), ptr(act_p), ptr(reward), R, B, M, N + 1, stream),
        [reward])
    # ---- PDP-100 -----------------------------------------------------------------------------------------------------------
    act_q = pdp_tours(R, gen)
    add("check_solution_pdp", lambda lib: lib.eamrl_check_solution(ops.ENVS["pdp"], ptr(act_q), None, None, R, R, N, N, ptr(bad), stream),
        [bad])
    # ---- OP-100: 40 customers, then the depot to the end -------------------------------------------------------------------
    act_o = torch.cat([perms(R, N, gen)[:, :40] + 1, torch.zeros(R, 10, dtype=torch.int64, device=DEV)], 1).contiguous()
    maxlen = torch.full((B, M), 100.0, device=DEV)
    add("op_check_solution", lambda lib: lib.eamrl_op_check_solution(ptr(act_o), ptr(locs_d), ptr(maxlen), R, B, M, 50, ptr(bad), stream),
        [bad])
    add("op_reward", lambda lib: lib.eamrl_op_reward(ptr(prize), ptr(act_o), ptr(reward), R, B, M, 50, stream), [reward])
    return rows


def ea_rows(libs, args):
    """EA.run through the binding, whose library handle is switched between the builds."""
    rows = {}
    shapes = [(e, N, B, 100, rates) for e in ("tsp", "cvrp", "pctsp", "op") for rates in ((0.1, 0.6, 0.2), (0.5, 0.9, 1.0))]
    shapes += [("tsp", 200, 64, 200, (0.1, 0.6, 0.2)), ("cvrp", 200, 64, 200, (0.1, 0.6, 0.2))]      # the device-memory path
    G = 3
    for env_name, n, b, S, rates in shapes:
        torch.manual_seed(11)
        env = ea.get_env(env_name, generator_params=dict(num_loc=n), seed=5)
        td = env.reset(batch_size=[b]).to(DEV)
        _lib._lib = libs["b"]
        pol = ea.AttentionModelPolicy(env_name=env_name).eval().to(DEV)
        with torch.no_grad():
            out = pol(td.clone(), env, phase="train", decode_type="multistart_sampling", num_starts=S)
        init = ea.unbatchify(out["actions"], S).contiguous()
        runner = ea.EA(env, dict(num_generations=G, mutation_rate=rates[0], crossover_rate=rates[1], selection_rate=rates[2]))
        gen = torch.Generator(device=DEV).manual_seed(100)
        if env_name == "tsp":
            d = ea.EADraws.sample(G, b, S, n, rates[2], DEV, gen)
        else:
            d = (ea.EACvrpDraws if env_name == "cvrp" else ea.EAPrizeDraws).sample(G, b, S, rates[2], DEV, gen)

        def call(lib):
            _lib._lib = lib
            return list(runner.run(init, td, draws=d))

        name = f"ea_{env_name}{n}_B{b}_S{S}_rates{'_'.join(str(x) for x in rates)}"
        rows[name], _ = ab_row(name, call, libs, args.rounds, args.window)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True)
    ap.add_argument("--b", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of launches per build and round")
    ap.add_argument("--rows", type=int, default=102400)
    ap.add_argument("--ea", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU timing"
    assert args.rows % B == 0 and args.rows >= 1024
    _lib.load()
    libs = {"a": load_lib(args.a), "b": load_lib(args.b)}
    rows = epilogue_rows(libs, args)
    if args.ea:
        rows.update(ea_rows(libs, args))
    out = {"what": f"{N}-node graphs, {B} instances, {args.rows} rows; {args.rounds} rounds, builds alternating, device events around "
                   f"{args.window} s of launches per build and round; pass: mean(b) <= mean(a) + (max(a) - min(a)), outputs bit-identical",
           "a": args.a, "b": args.b, "rows": rows, "all_pass": all(r["pass"] for r in rows.values())}
    print(json.dumps({"all_pass": out["all_pass"], "failed": [k for k, r in rows.items() if not r["pass"]]}))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
