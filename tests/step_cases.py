"""Hand-built instances that put a row of every routing env ON a comparison boundary of its step-and-mask rule, and the
scripts that drive the row there.

A case is B = 3 instances with different data (so that a wrong instance index on a per-instance tensor shows once rows of
several starts share them) and, per instance, the `heads` of its rows' preference lists: heads[b][t] are the nodes a row of
instance b tries first at step t; after them come all nodes in a seeded order (`prefs`).  A row takes the first node of its
list that its mask allows (step_ref.rollout_first_feasible), so a boundary node put first is taken exactly when the rule
judges it feasible -- a copy of the rule that judges it differently takes a different action.

Every boundary value is built in float32 arithmetic and the builder asserts what the float32 comparison gives: "one step
above" is found by walking float32 neighbours until the rounded sum actually changes (0.5 + nextafter(lim - 0.5) still
rounds back to lim).  `verdicts` name what each case claims, as (b, t, kind, arg, expected, label):
    kind "mask": node `arg` is feasible (or not) in the state after t actions;  "done": the row's done flag;
    "slot": the float32 / integer state slot `arg` equals `expected` exactly.
tests/test_host_step_ref.py asserts them on states recorded from the reference.

`padded(case, M)` moves the named customers 1, 2, 3 to the node indices 63, 64 and M - 1 (the rest behind them) of a graph
of M nodes and fills the other nodes with plain customers: the sizes at which the kernels change their node-to-lane layout
or stop being chosen (65: second node slot per lane of the resident kernel; 112 / 113: last size of the start-sharing MFMA
kernel and of the one-chunk replay layout; 128 / 129: last size of the resident kernel; 257: block-stride loops).

What cannot be a case, because it leaves a row without any feasible action: a CVRPTW customer that is free by capacity but
late while the vehicle stands at the depot (the clock is 0 there, so it is late for ever and the depot stays masked), and a
PCTSP depot visit at step 0 (the depot is masked until the prize is collected).  The CVRPTW late customer is therefore met
from another customer, and the `i == 0` depot visit is OP's.
"""
from __future__ import annotations

import zlib

import numpy as np

from eam_rl4co_amd import env_spec

f32 = np.float32
LIM = f32(f32(1.0) + f32(1e-5))          # vehicle_capacity + 1e-5 of the CVRP mask, one float32 add
assert LIM == f32(1.0) + f32(84 * 2.0 ** -23)


def walk(x, toward, until):
    """The first float32 on the way from x toward `toward` (x excluded) for which until(value) holds."""
    x = f32(x)
    for _ in range(64):
        x = np.nextafter(x, f32(toward))
        if until(x):
            return x
    raise AssertionError("no such float32 within 64 steps")


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def prefs(case, S, T=None):
    """[R, T, M] int64 for R = S * B rows (row r: instance r % B): the case's heads, then every other node in an order seeded
    by (case, row, step)."""
    M, B = case["M"], 3
    T = T or env_spec.max_steps(env_spec.spec(case["env"]).name, M)
    out = np.empty((S * B, T, M), np.int64)
    for r in range(S * B):
        heads = case["heads"][r % B]
        for t in range(T):
            head = list(heads[t]) if t < len(heads) else []
            rest = np.random.default_rng(_seed(case["name"], r, t)).permutation(M)
            out[r, t] = head + [n for n in rest if n not in head]
    return out


def noise_from_prefs(p):
    """noise[r, t, n] = (1 + rank of n in prefs[r, t]) / M: with equal log-probabilities the kernels' sampling key
    exp(lp) / noise picks the feasible node of the smallest noise, i.e. the first feasible node of the list."""
    R, T, M = p.shape
    rank = np.empty_like(p)
    np.put_along_axis(rank, p, np.broadcast_to(np.arange(M), p.shape), axis=-1)
    return ((1 + rank).astype(np.float64) / M).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
U = 8.0                     # CVRPTW grid unit: legs of the scripts are axis-parallel or 3-4-5, so they are exact


def _grid(points, unit):
    return (np.array(points, np.float64) * unit).astype(f32)


def _cvrp_like_batch(env, demand, extra=None):
    demand = np.array(demand, f32)
    B, N = demand.shape
    rng = np.random.default_rng(_seed(env, "locs"))
    batch = {"env": env, "depot": rng.random((B, 2)).astype(f32), "locs": rng.random((B, N, 2)).astype(f32), "demand": demand}
    batch.update(extra or {})
    return batch


def _case(name, env, batch, heads, verdicts):
    M = batch["locs"].shape[1] + (env != "tsp")
    return {"name": name, "env": env, "M": M, "batch": batch, "heads": heads, "verdicts": verdicts}


def _cvrp_lim():
    half = f32(0.5)
    at = f32(LIM - half)
    assert f32(half + at) == LIM                                           # exact: feasible
    above = walk(at, 2.0, lambda d: f32(half + d) > LIM)
    assert above != np.nextafter(at, f32(2)) and f32(half + np.nextafter(at, f32(2))) == LIM   # the neighbour rounds back
    below = walk(at, 0.0, lambda d: f32(half + d) < LIM)
    demand = [[0.5, at, 0.25, 0.25, 0.125, 0.0, 0.0625, 0.75],
              [0.5, above, 0.125, 0.3, 0.2, 0.1, 0.0625, 0.7],
              [0.5, below, 0.0625, 0.15, 0.45, 0.05, 0.6, 0.35]]
    heads = [[[1], [2]], [[1], [2, 3]], [[1], [2]]]
    verdicts = [(0, 0, "mask", 0, False, "the depot, at the depot, while customers are free"),
                (0, 1, "mask", 2, True, "load == vcap + 1e-5"),
                (1, 1, "mask", 2, False, "load one float32 step above vcap + 1e-5"),
                (2, 1, "mask", 2, True, "load one float32 step below vcap + 1e-5"),
                (0, 1, "mask", 0, True, "the depot, at a customer"),
                (0, 2, "mask", 6, True, "zero demand on a load of vcap + 1e-5"),
                (0, 2, "mask", 7, False, "the smallest positive demand on a load of vcap + 1e-5"),
                (0, 2, "slot", "used", LIM, "used == vcap + 1e-5")]
    return demand, heads, verdicts


def _cvrp_vcap():
    # b0: 0.5 + 0.5 == vcap, then only the zero-demand customer and the depot; b1: eight times 1/8 == vcap in ONE trip, the
    # depot is visited last and only then the row is done; b2: one trip per customer (the first one's demand == vcap), the
    # depot has been visited when the last customer is, so the row is done there -- and keeps choosing the depot
    demand = [[0.5, 0.5, 0.0, 0.25, 0.125, 0.0625, 0.375, 0.625],
              [0.125] * 8,
              [1.0, 0.75, 0.75, 0.875, 0.75, 0.625, 0.75, 0.75]]
    heads = [[[1], [2], [4, 3], [5, 0]],
             [[n] for n in range(1, 9)] + [[0]],
             [[1], [2, 0]] + [[n] for k in range(2, 9) for n in (k, 0)]]
    verdicts = [(0, 2, "mask", 3, True, "zero demand on a full vehicle"),
                (0, 2, "slot", "used", f32(1.0), "used == vcap"),
                (0, 2, "mask", 4, False, "positive demand on a full vehicle"),
                (0, 2, "mask", 0, True, "the depot, at a customer"),
                (0, 3, "mask", 0, True, "the depot, at a customer, while no customer is free"),
                (0, 3, "mask", 5, False, "no customer is free"),
                (1, 8, "done", None, False, "all customers visited, the depot not yet"),
                (1, 8, "mask", 0, True, "the depot while no customer is free"),
                (1, 9, "done", None, True, "the depot visited last"),
                (1, 9, "mask", 0, True, "the depot again, everything blocked"),
                (2, 0, "mask", 1, True, "demand == vcap"),
                (2, 1, "mask", 2, False, "full vehicle"),
                (2, 15, "done", None, True, "the last customer, the depot visited before"),
                (1, 10, "mask", 0, True, "the depot twice in a row once everything is blocked")]
    return demand, heads, verdicts


def cvrp_cases():
    for name, build in (("cvrp_lim", _cvrp_lim), ("cvrp_vcap", _cvrp_vcap)):
        demand, heads, verdicts = build()
        yield _case(name, "cvrp", _cvrp_like_batch("cvrp", demand), heads, verdicts)


def _tw_extra(points, tw, dur):
    """CVRPTW's tensors from grid points [B][M] (depot first), windows [B][M][2] and durations [B][M]."""
    locs = np.stack([_grid(p, U) for p in points])
    return {"depot": locs[:, 0].copy(), "locs": locs[:, 1:].copy(), "time_windows": np.array(tw, np.int32),
            "durations": np.array(dur, f32)}


FAR = 1 << 20               # a window end nobody misses (the depot's: every reachable state must be able to return)


def cvrptw_cases():
    # capacity boundaries, clock idle: every node at the depot's place would make legs 0; put them on the grid with wide windows
    pts = [[(0, 0)] + [(k % 3, k // 3) for k in range(1, 9)]] * 3
    wide = [[[0, FAR]] * 9] * 3
    for name, build in (("cvrptw_lim", _cvrp_lim), ("cvrptw_vcap", _cvrp_vcap)):
        demand, heads, verdicts = build()
        batch = _cvrp_like_batch("cvrptw", demand)
        batch.update(_tw_extra(pts, wide, [[0.0] + [1.0 + b] * 8 for b in range(3)]))
        yield _case(name, "cvrptw", batch, heads, verdicts)

    # the clock.  depot (0,0); 1 = (3,0): leg 24; 2 = (3,4): leg 32 from node 1, 40 from the depot; 3 = (0,4): leg 32 from
    # the depot, 24 from node 2; 4 = (6,8): 80 from the depot
    pts = [[(0, 0), (3, 0), (3, 4), (0, 4), (6, 8), (1, 0), (0, 1)]] * 3
    d_at = f32(4.0)
    assert f32(f32(f32(24.0) + d_at) + f32(32.0)) == f32(60.0)
    d_late = walk(d_at, 8.0, lambda d: f32(f32(f32(24.0) + d) + f32(32.0)) > f32(60.0))
    assert d_late != np.nextafter(d_at, f32(8))          # the neighbour still arrives at 60
    #            depot      1          2         3          4           5          6
    tw = [[[0, FAR], [0, 100], [10, 60], [0, 400], [0, 100], [0, FAR], [0, FAR]],      # b0: arrives at 2 at its window's end
          [[0, FAR], [0, 100], [10, 60], [0, 400], [0, 100], [0, FAR], [0, FAR]],      # b1: one float32 step later
          [[0, FAR], [24, 100], [70, 90], [32, 400], [0, 100], [0, FAR], [0, FAR]]]    # b2: at node 1's start; before node 2's
    dur = [[0, d_at, 5, 2, 1, 1, 1], [0, d_late, 5, 2, 1, 1, 1], [0, 4, 5, 200, 1, 1, 1]]
    demand = [[0.125] * 6, [0.25, 0.125, 0.125, 0.125, 0.125, 0.125], [0.125, 0.25, 0.125, 0.0625, 0.125, 0.125]]
    heads = [[[1], [2], [3], [0]], [[1], [2, 3], [0]], [[1], [2], [3], [4, 0]]]
    verdicts = [(0, 1, "slot", "time", f32(28.0), "arrival inside the window: clock = arrival + duration"),
                (0, 1, "mask", 2, True, "arrival == the window's end"),
                (1, 1, "mask", 2, False, "arrival one float32 step after the window's end"),
                (1, 1, "mask", 3, True, "a later window"),
                (0, 2, "slot", "time", f32(65.0), "service started at the window's end"),
                (0, 4, "slot", "time", f32(0.0), "the depot zeroes the clock"),
                (2, 1, "slot", "time", f32(28.0), "arrival == the window's start"),
                (2, 2, "slot", "time", f32(75.0), "arrival before the window's start: the clock jumps to it"),
                (2, 3, "slot", "time", f32(299.0), "99 + 200"),
                (2, 3, "mask", 4, False, "free by capacity but late (seen from a customer)"),
                (2, 3, "mask", 0, True, "the depot, at a customer"),
                (2, 4, "mask", 4, True, "the late customer, reachable again from the depot at time 0"),
                (2, 4, "mask", 0, False, "the depot, at the depot, while a customer is free")]
    batch = _cvrp_like_batch("cvrptw", demand)
    batch.update(_tw_extra(pts, tw, dur))
    yield _case("cvrptw_clock", "cvrptw", batch, heads, verdicts)


def sdvrp_cases():
    # b0: the remaining demand equals the free capacity: node emptied, vehicle filled in one step; b1: a split delivery;
    # b2: a node without demand from the start, one trip, done on the last delivery (no depot visit)
    demand = [[0.5, 0.5, 0.3, 0.25, 0.7, 0.125],
              [0.75, 0.5, 0.2, 0.25, 0.6, 0.375],
              [0.125, 0.25, 0.0, 0.125, 0.25, 0.125]]
    heads = [[[1], [2], [3, 0]], [[1], [2], [2, 0], [2]], [[1], [2], [3, 4], [5], [6]]]
    verdicts = [(0, 2, "slot", "used", f32(1.0), "used == vcap"),
                (0, 2, "mask", 2, False, "emptied"), (0, 2, "mask", 3, False, "used == vcap blocks every customer"),
                (0, 2, "mask", 0, True, "the depot"), (0, 3, "mask", 3, True, "after the depot"),
                (1, 2, "slot", "used", f32(1.0), "split delivery fills the vehicle"),
                (1, 2, "mask", 2, False, "demand left, vehicle full"), (1, 3, "mask", 2, True, "the rest of the split demand"),
                (1, 4, "slot", "used", f32(0.25), "the rest delivered"),
                (2, 0, "mask", 3, False, "no demand from the start"), (2, 0, "mask", 0, False, "the depot, customers free"),
                (2, 4, "done", None, False, "one delivery left"), (2, 5, "done", None, True, "done on the last delivery"),
                (2, 5, "mask", 0, True, "the depot, nothing left"), (2, 6, "mask", 0, True, "the depot again")]
    yield _case("sdvrp_split", "sdvrp", _cvrp_like_batch("sdvrp", demand), heads, verdicts)


def pctsp_cases(env="pctsp"):
    quarter = f32(0.25)
    below = walk(quarter, 0.0, lambda p: f32(f32(0.75) + p) < f32(1.0))
    assert below != np.nextafter(quarter, f32(0)) and f32(f32(0.75) + np.nextafter(quarter, f32(0))) == f32(1.0)
    real = np.array([[0.5, 0.25, 0.25, 0.125, 0.375, 0.125, 0.25, 0.125],
                     [0.5, 0.25, below, 0.125, 0.375, 0.125, 0.25, 0.125],
                     [0.0625] * 8], f32)
    rng = np.random.default_rng(_seed(env, "other"))
    other = (rng.random(real.shape) * 0.3).astype(f32)                 # the prize the rule must NOT read
    batch = {"env": env, "depot": rng.random((3, 2)).astype(f32), "locs": rng.random((3, 8, 2)).astype(f32),
             "penalty": (rng.random(real.shape) * 0.1).astype(f32),
             "deterministic_prize": other if env == "spctsp" else real, "stochastic_prize": real if env == "spctsp" else other}
    heads = [[[0, 1], [0, 2], [0, 3], [0]], [[0, 1], [0, 2], [0, 3], [0, 4], [0]], [[0, n] for n in range(1, 9)] + [[0]]]
    verdicts = [(0, 0, "mask", 0, False, "the depot at step 0"), (0, 2, "mask", 0, False, "prize 0.75"),
                (0, 3, "slot", "used", f32(1.0), "prize total == 1.0"), (0, 3, "mask", 0, True, "prize total == 1.0"),
                (0, 4, "done", None, True, "the depot later"), (0, 4, "mask", 4, False, "after the depot every customer is masked"),
                (0, 4, "mask", 0, True, "the depot again"),
                (1, 3, "slot", "used", np.nextafter(f32(1.0), f32(0)), "prize total one float32 step below 1.0"),
                (1, 3, "mask", 0, False, "prize total one float32 step below 1.0"), (1, 4, "mask", 0, True, "prize above 1"),
                (2, 7, "mask", 0, False, "one customer left, prize below 1"),
                (2, 8, "mask", 0, True, "all customers visited, prize 0.5"), (2, 9, "done", None, True, "the depot")]
    yield _case(env + "_prize", env, batch, heads, verdicts)


def _op_unit():
    """A grid unit u = k / 128 for which both arrival limits of op_cases exist: `max_length - back - 1e-6` rounds twice, so
    not every float32 is the limit of some max_length."""
    for k in range(8, 64):
        u = k / 128.0
        try:
            _op_total_for(f32(7 * u), f32(5 * u))
            _op_total_for(np.nextafter(f32(7 * u), f32(0)), f32(5 * u))
            return u
        except AssertionError:
            continue
    raise AssertionError("no grid unit found")


def _op_limit(total, back):
    """OPEnv._reset's arrival limit of a node `back` away from the depot, in float32."""
    return f32(f32(f32(total) - f32(back)) - f32(1e-6))


def _op_total_for(limit, back):
    """A max_length whose arrival limit for that node is exactly `limit` (not every value can be hit: the caller picks one)."""
    guess = f32(f32(f32(limit) + f32(back)) + f32(1e-6))
    x = guess
    for _ in range(8):
        x = np.nextafter(x, f32(0))
    for _ in range(32):
        if _op_limit(x, back) == f32(limit):
            return x
        x = np.nextafter(x, f32(4))
    raise AssertionError(f"no max_length gives the arrival limit {limit!r}")


OP_U = _op_unit()           # OP grid unit


def op_cases():
    # depot (0,0); 1 = (3,0): 3 u away; 2 = (3,4): 5 u from the depot, 4 u from node 1: arriving there after node 1 makes
    # tour_len + leg = 7 u.  3 = (0,4), 4 = (6,8): 10 u away, out of reach; 5, 6 near the depot
    pts = [(0, 0), (3, 0), (3, 4), (0, 4), (6, 8), (1, 0), (0, 1)]
    locs = _grid(pts, OP_U)
    arrive, back = f32(7 * OP_U), f32(5 * OP_U)
    total_at = _op_total_for(arrive, back)
    total_above = _op_total_for(np.nextafter(arrive, f32(0)), back)      # the limit one step under the arrival
    assert _op_limit(total_at, back) == arrive and not (arrive > _op_limit(total_at, back))
    assert arrive > _op_limit(total_above, back) and np.nextafter(_op_limit(total_above, back), f32(1)) == arrive
    batch = {"env": "op", "depot": np.stack([locs[0]] * 3), "locs": np.stack([locs[1:]] * 3),
             "prize": np.array([[1, 2, 3, 4, 5, 6], [2, 1, 1, 3, 1, 1], [1, 1, 2, 1, 3, 1]], f32) / 8,
             "max_length": np.array([total_at, total_above, 2.0], f32)}
    heads = [[[5], [1], [2, 3], [0]], [[5], [1], [2, 3], [0]], [[0], [1, 0]]]      # (via node 5: 1 u + 2 u, still exact)
    verdicts = [(0, 2, "slot", "used", f32(3 * OP_U), "exact legs"),
                (0, 2, "mask", 2, True, "tour_len + leg == max_length[n]"),
                (1, 2, "mask", 2, False, "tour_len + leg one float32 step above max_length[n]"),
                (0, 3, "slot", "used", f32(7 * OP_U), "arrived at the limit"),
                (0, 2, "mask", 4, False, "out of reach"), (0, 0, "mask", 0, True, "the depot is always feasible"),
                (0, 2, "mask", 0, True, "the depot is always feasible"),
                (2, 1, "done", None, False, "the depot at i == 0 is not done"),
                (2, 1, "mask", 1, False, "the depot visited blocks all customers"),
                (2, 1, "mask", 0, True, "the depot is always feasible"),
                (2, 2, "done", None, True, "the depot at i > 0")]
    yield _case("op_length", "op", batch, heads, verdicts)
    # every row visits the depot at i == 0: not done, so the batch takes a second step (a copy that calls the first visit done
    # ends the rollout one step early -- with a single such row among longer ones nothing else would show, since all a row can
    # do afterwards is to choose the depot again)
    batch = dict(batch, prize=batch["prize"][::-1].copy(), max_length=np.array([2.0, total_at, 1.0], f32))
    verdicts = [(b, 1, what, arg, expected, label) for b in range(3) for what, arg, expected, label in
                (("done", None, False, "the depot at i == 0 is not done"), ("mask", 5, False, "the depot visited blocks all customers"),
                 ("mask", 0, True, "the depot is always feasible"))] + [(0, 2, "done", None, True, "the depot at i > 0")]
    yield _case("op_depot_first", "op", batch, [[[0]], [[0]], [[0]]], verdicts)


def tsp_cases():
    rng = np.random.default_rng(_seed("tsp"))
    yield _case("tsp_two", "tsp", {"env": "tsp", "locs": rng.random((3, 2, 2)).astype(f32)}, [[[1]], [[0]], [[1], [0]]],
                [(0, 1, "done", None, False, "one node left"), (0, 1, "mask", 1, False, "visited"),
                 (0, 2, "done", None, True, "the last node"), (1, 1, "slot", "first", 0, "first node")])
    yield _case("tsp_five", "tsp", {"env": "tsp", "locs": rng.random((3, 5, 2)).astype(f32)},
                [[[4], [0]], [[2]], [[3], [3, 1]]],
                [(0, 4, "done", None, False, "one node left"), (0, 5, "done", None, True, "the last node"),
                 (0, 2, "slot", "first", 4, "the first node stays"), (2, 1, "mask", 3, False, "visited")])


def pdp_cases():
    # PDP has no float rule: pdp_ref's state machine on N = 6 (pickups 1-3, deliveries 4-6)
    rng = np.random.default_rng(_seed("pdp"))
    batch = {"env": "pdp", "depot": rng.random((3, 2)).astype(f32), "locs": rng.random((3, 6, 2)).astype(f32)}
    heads = [[[4, 1], [4]], [[6, 3], [1], [6]], [[0, 5, 2], [5]]]
    verdicts = [(0, 0, "mask", 4, False, "a delivery before its pickup"), (0, 0, "mask", 0, False, "the depot"),
                (0, 1, "mask", 4, True, "the delivery of the pickup just made"), (0, 1, "mask", 5, False, "another delivery"),
                (1, 1, "mask", 6, True, "pickup 3 opens delivery 6"), (0, 6, "done", None, True, "every node visited")]
    yield _case("pdp_pairs", "pdp", batch, heads, verdicts)


def named_cases():
    """Every named case, in a fixed order."""
    out = []
    for gen in (tsp_cases, cvrp_cases, cvrptw_cases, sdvrp_cases, pctsp_cases, lambda: pctsp_cases("spctsp"), op_cases,
                pdp_cases):
        out.extend(gen())
    return out


NAMES = ["tsp_two", "tsp_five", "cvrp_lim", "cvrp_vcap", "cvrptw_lim", "cvrptw_vcap", "cvrptw_clock", "sdvrp_split", "pctsp_prize",
         "spctsp_prize", "op_length", "op_depot_first", "pdp_pairs"]
# per case ((b, k, node) feasible, (b, k, node) infeasible): the two sides of the case's boundary in the state after k steps; the
# feasible node is the action the script takes there
BOUNDARY_PAIRS = {"cvrp_lim": ((0, 1, 2), (1, 1, 2)), "cvrp_vcap": ((0, 1, 2), (0, 2, 4)), "cvrptw_lim": ((0, 1, 2), (1, 1, 2)),
                  "cvrptw_vcap": ((0, 1, 2), (0, 2, 4)),
                  "cvrptw_clock": ((0, 1, 2), (1, 1, 2)), "sdvrp_split": ((0, 1, 2), (0, 2, 3)),
                  "pctsp_prize": ((0, 3, 0), (1, 3, 0)), "spctsp_prize": ((0, 3, 0), (1, 3, 0)), "op_length": ((0, 2, 2), (1, 2, 2))}
PADDED_M = (65, 112, 113, 128, 129)
BIG_M = 257                 # stand-alone step and replay kernels only, TSP and CVRP


def case_by_name(name):
    return {c["name"]: c for c in named_cases()}[name]


# ---------------------------------------------------------------------------------------------------------------------
# padded variants
# ---------------------------------------------------------------------------------------------------------------------
def node_map(n_named, M):
    """New index of the named nodes 0 .. n_named - 1 (node 0 stays; customers 1, 2, 3 go to 63, 64, M - 1)."""
    want = [63, 64, M - 1, 62, 65, M - 2, 61, 66, M - 3, 60, 67, M - 4] + list(range(59, 40, -1))
    seen, targets = {0}, []
    for w in want:
        if 0 < w < M and w not in seen:
            seen.add(w)
            targets.append(w)
    return np.array([0] + targets[:n_named - 1], np.int64)


def padded(case, M):
    """The case on a graph of M nodes: its named nodes moved by `node_map`, every other node a plain customer whose data
    differ by instance.  PDP (paired nodes) and TSP (no boundary) only grow: seeded preferences on M nodes."""
    env = case["env"]
    rng = np.random.default_rng(_seed("pad", case["name"], M))
    if env == "tsp":
        return _case(f"{case['name']}_m{M}", env, {"env": env, "locs": rng.random((3, M, 2)).astype(f32)}, case["heads"], [])
    if env == "pdp":
        assert M % 2 == 1
        return _case(f"{case['name']}_m{M}", env, {"env": env, "depot": rng.random((3, 2)).astype(f32),
                                                  "locs": rng.random((3, M - 1, 2)).astype(f32)}, [[], [], []], [])
    old = case["batch"]
    n_named = case["M"]
    nm = node_map(n_named, M)
    cust = nm[1:] - 1                          # customer slots (arrays without the depot)
    batch = {"env": env, "depot": old["depot"].copy()}
    inst = np.arange(3, dtype=np.float64)[:, None]

    def fill(key, filler, with_depot=False):
        v = np.array(np.broadcast_to(filler, (3, M if with_depot else M - 1) + old[key].shape[2:]), dtype=old[key].dtype)
        if with_depot:
            v[:, nm] = old[key]
        else:
            v[:, cust] = old[key]
        batch[key] = v

    k = np.arange(M - 1)
    if env in ("cvrp", "sdvrp", "cvrptw"):
        fill("demand", ((1 + inst) / 512).astype(f32))
    if env == "cvrptw":
        grid = np.stack([(k % 9) * U, (k % 7) * U], -1).astype(f32)
        fill("locs", grid[None])
        fill("time_windows", np.array([0, FAR], np.int32), with_depot=True)
        fill("durations", f32(1.0), with_depot=True)
    elif env == "op":
        grid = np.stack([(k % 5) * OP_U, (k % 3) * OP_U], -1).astype(f32)
        fill("locs", grid[None])
        fill("prize", f32(0.125))
        batch["max_length"] = old["max_length"].copy()
    else:
        fill("locs", rng.random((3, M - 1, 2)).astype(f32))
    if env in ("pctsp", "spctsp"):
        for key in ("deterministic_prize", "stochastic_prize", "penalty"):
            fill(key, ((1 + inst) / 1024).astype(f32))
    heads = [[[int(nm[n]) for n in step] for step in rows] for rows in case["heads"]]
    return _case(f"{case['name']}_m{M}", env, batch, heads, [])
