"""What test_host_validity.py and test_gpu_validity.py share: the committed fixtures with the restatement's result next
to each group (computed once, read-only), the counters that the recorded verdicts imply, and the cases built on top of
the fixtures (multistart layout, the wide CVRP graph)."""
import os

import numpy as np

import make_golden_validity as mk
import validity_ref as vr
from _util import GOLDEN

ENVS = ("tsp", "cvrp", "sdvrp", "pctsp", "op", "cvrptw")
_cache = {}


def fixture(env):
    """The groups of validity_<env>.npz with the restatement's Result next to each (`ref`), computed once and shared."""
    if env not in _cache:
        groups = mk.load_groups(os.path.join(GOLDEN, f"validity_{env}.npz"))
        for g in groups:
            g["ref"] = mk.evaluate(env, g)
            for v in g.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _cache[env] = groups
    return _cache[env]


def expected_counters(env, g):
    """[R, K] what each row adds to the kernels' counters, from the RECORDED verdict.  SDVRP replays a row to its end and
    the CVRPTW time replay runs apart from the CVRP check, so there the restatement says whether a row that already
    failed is counted a second time; what the recorded verdict fixes is asserted here."""
    v, c = g["verdict"], g["ref"].counters
    if env in ("tsp", "cvrp", "pctsp", "op"):
        return np.stack([v == 1, v == 2], axis=1).astype(np.int64)
    if env == "sdvrp":
        assert np.array_equal(c[:, 1] == 1, v == vr.DEPOT_TWICE)
        assert np.array_equal((c[:, 0] == 1) & (c[:, 1] == 0), v == vr.DEMAND_LEFT)
        return c
    assert np.array_equal(c[:, 0] == 1, v == vr.INVALID_TOUR) and np.array_equal(c[:, 1] == 1, v == vr.OVER_CAPACITY)
    assert np.array_equal((c == (0, 0, 1)).all(axis=1), v == vr.LATE)
    return c


def top_id(env, g):
    """The highest legal node id of a group."""
    if env == "tsp":
        return g["actions"].shape[1] - 1
    return {"cvrp": lambda: g["demand"].shape[1], "sdvrp": lambda: g["demand"].shape[1],
            "pctsp": lambda: g["real_prize"].shape[1] - 1, "op": lambda: g["locs"].shape[1] - 1,
            "cvrptw": lambda: g["locs"].shape[1] - 1}[env]()


def multistart_case(env, S, group=1):
    """S * B rows in "(s b)" order against B distinct instances of one fixture group: row r belongs to instance r % B.
    Even s: a tour that is valid for its own instance; odd s: a valid tour of the NEXT instance, which this one judges
    by its own data.  -> (instance arrays [B, ...] as a group dict, actions [S * B, T], Result of the restatement with
    the r % B mapping, Result with the wrong r // S mapping)."""
    g = fixture(env)[group]
    has_valid = sorted(set(g["inst"][g["verdict"] == 0].tolist()))
    pick = sorted(has_valid, key=lambda b: not mk.representable(env, g, b))[:3]
    B = len(pick)
    assert B == 3
    sub = {k: g[k][pick] for k in mk.INSTANCE_KEYS[env]}
    rows = []
    for s in range(S):
        for b in range(B):
            owner = pick[(b + s % 2) % B]
            mine = np.flatnonzero((g["inst"] == owner) & (g["verdict"] == 0))
            rows.append(g["actions"][mine[s % mine.size]])
    actions = np.stack(rows)
    sub["actions"], sub["inst"] = actions, np.arange(S * B) % B
    right = mk.evaluate(env, sub)
    wrong = mk.evaluate(env, sub, inst=np.arange(S * B) // S)
    return sub, actions, right, wrong


def wide_cvrp_case():
    """1000 customers, demands in units of 1/64, about 1100 steps: a valid row, customer 999 twice, customer 1000 missing,
    and a row overloaded in its last route only."""
    rng = np.random.default_rng(1000)
    N = 1000
    raw = rng.integers(1, 17, size=N)
    routes = mk.routes_for(rng, raw, 64, 0)
    tour = mk.flat(routes)
    moved = mk.flat(mk.overload(rng, routes, raw, 64, -1))
    assert mk.first_over_step(moved, raw, 64) > 1000
    T = len(tour) + 3
    pad = lambda t: t + [0] * (T - len(t))
    actions = np.array([pad(tour), pad(tour + [999]), pad([0 if a == 1000 else a for a in tour]), pad(moved)], dtype=np.int64)
    demand = np.broadcast_to((raw / 64.0).astype(np.float32), (4, N)).copy()
    return demand, np.ones(4, np.float32), actions
