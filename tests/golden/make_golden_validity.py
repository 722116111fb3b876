#!/usr/bin/env python3
"""Fixtures for the solution-validity kernels, with verdicts recorded by RUNNING THE REFERENCE's own
`check_solution_validity` (tsp/env.py:161-168, cvrp/env.py:157-185, sdvrp/env.py:137-159, pctsp/env.py:180-204,
op/env.py:178-209, cvrptw/env.py:180-214) on the CPU, one row at a time, in the build container:

    python tests/golden/make_golden_validity.py

Every row is a feasible tour built here in numpy with exactly one corruption applied (its class label is stored next to
it), or an untouched valid tour.  The reference is called per row with that row's own instance; an AssertionError is
caught and its message recorded as the verdict code of tests/validity_ref.py.  Rows with ids out of range are not made
here (the reference would raise an IndexError); they live in tests/test_gpu_validity.py.

Verdicts are compared exactly, so no row may depend on the order of a float32 sum: tests/validity_ref.py gives every row
its decisive margin in float64, and `check_margins` (also run by tests/test_host_validity.py on the committed files)
asserts that it is at least 1e-3 or that the row is marked `exact` and its instance holds only numbers that float32 adds
exactly (small multiples of 1/64 or 1/1024; CVRP demands that are multiples of 2^-23 up to 1; integer coordinates,
windows and durations).  Nothing is dropped: a row that misses this fails the build of the fixtures.

NODES counts CUSTOMERS.  TSP has that many nodes; the depot envs have one node more (4, 21, 34, 65, 66, 101, 130, 301),
so customer ids and steps on both sides of 31/32, 63/64 and 127/128 occur in every env.

One `validity_<env>.npz` per env holds groups g0, g1, ... of one shape each: `gK_actions` [R, T], `gK_inst` [R] (the
row's instance), `gK_verdict`, `gK_cls`, `gK_exact`, and the instance arrays `gK_<name>` [B, ...].  Only data is stored.
The archive is written with fixed time stamps, so a rerun gives the same bytes.
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import validity_ref as vr  # noqa: E402

NODES = (3, 20, 33, 64, 65, 100, 129, 300)      # customers per group: both sides of 32, 64 and 128, and a wide one
MARGIN = 1e-3
ULP = 2.0 ** -23                                # float32(1 + 1e-5) is 1 + 84 ULP: the capacity limit of a vehicle of capacity 1
INSTANCE_KEYS = {"tsp": (), "cvrp": ("demand", "capacity"), "sdvrp": ("demand", "capacity"), "pctsp": ("real_prize",),
                 "op": ("locs", "max_length"), "cvrptw": ("locs", "demand", "capacity", "time_windows", "durations")}
# the classes the fixtures must hold (test_host_validity.py checks them from the stored labels)
CLASSES = {
    "tsp": ("valid", "dup_pos0", "dup_pos63", "dup_pos64", "dup_poslast", "dup_id31", "dup_id32", "dup_id63", "dup_id64"),
    "cvrp": ("valid", "twice", "missing", "over_last", "over_step64", "over_first", "merge", "exact_full", "exact_over",
             "exact_at_limit", "exact_ulp_over"),
    "sdvrp": ("valid", "left", "start_twice", "end_twice_valid", "revisit_valid", "twice_and_left", "no_depot"),
    "pctsp": ("valid", "dup", "short", "short_all_visited", "only_depot", "exact_one", "exact_short"),
    "op": ("valid", "dup", "too_long", "repeat_depot_valid"),
    "cvrptw": ("valid", "late_first", "late_after_reset", "late_step64", "wait_valid", "exact_end", "exact_one_late",
               "twice", "missing", "over_last", "over_step64", "over_first", "merge"),
}


# ---------------------------------------------------------------------------------------------------------
# the restatement on a fixture group, and the margin guarantee (shared with the tests)
# ---------------------------------------------------------------------------------------------------------
def evaluate(env, g, actions=None, inst="own"):
    """validity_ref on the rows of a group (a dict with the instance arrays, `actions` and `inst`)."""
    a = g["actions"] if actions is None else actions
    i = g["inst"] if isinstance(inst, str) else inst
    if env == "tsp":
        return vr.tsp(a)
    return getattr(vr, env)(*[g[k] for k in INSTANCE_KEYS[env]], a, inst=i)


def _on_grid(x, unit):
    """Multiples of 1 / unit, small enough that float32 holds any sum of a row's worth of them exactly."""
    x = np.asarray(x, np.float64) * unit
    return bool((x == np.round(x)).all() and (np.abs(x) < 2 ** 14).all())


def _on_ulp_grid(x):
    """Multiples of 2^-23 in [0, 1].  The load replay adds them in step order; with capacity 1 every load below 2 is then
    exact in float32, as is the depot's load - 1, and a load of 2 or more is over the limit however it is rounded."""
    x = np.asarray(x, np.float64) / ULP
    return bool((x == np.round(x)).all() and (x >= 0).all() and (x <= 2 ** 23).all())


def representable(env, g, b):
    """Instance b of the group holds only numbers on which the float32 replay is exact."""
    if env == "cvrp":
        return _on_ulp_grid(g["demand"][b]) and float(g["capacity"][b]) == 1.0
    if env == "sdvrp":
        return _on_grid(g["demand"][b], 1024) and float(g["capacity"][b]) == 1.0
    if env == "pctsp":
        return _on_grid(g["real_prize"][b], 64)
    if env == "cvrptw":
        return (_on_grid(g["demand"][b], 64) and float(g["capacity"][b]) == 1.0 and _on_grid(g["locs"][b], 1)
                and _on_grid(g["durations"][b], 1) and _on_grid(g["time_windows"][b], 1))
    return env == "tsp"


def check_margins(env, g, res=None):
    """Every row: margin >= 1e-3, or marked exact on a representable instance.  CVRPTW additionally lives on integer
    grids throughout (validity_ref leaves exactly integral arrival times out of the margin)."""
    res = evaluate(env, g) if res is None else res
    for r in range(g["actions"].shape[0]):
        b = int(g["inst"][r])
        if env == "cvrptw":
            assert _on_grid(g["locs"][b], 1) and _on_grid(g["durations"][b], 1) and _on_grid(g["time_windows"][b], 1)
        if res.margin[r] >= MARGIN:
            continue
        assert bool(g["exact"][r]) and representable(env, g, b), \
            f"{env} row {r} ({g['cls'][r]}): margin {res.margin[r]:.3g} and not exactly representable"
    return res


# ---------------------------------------------------------------------------------------------------------
# row builders
# ---------------------------------------------------------------------------------------------------------
class Group:
    def __init__(self):
        self.inst = {}
        self.rows = []              # (instance index, list of actions, class)

    def add_instance(self, **arrays):
        for k, v in arrays.items():
            self.inst.setdefault(k, []).append(v)
        return len(next(iter(self.inst.values()))) - 1

    def add(self, b, actions, cls):
        self.rows.append((b, [int(x) for x in actions], cls))


def routes_for(rng, raw, capraw, headroom):
    routes, cur, load = [], [], 0
    for c in rng.permutation(len(raw)) + 1:
        if cur and load + raw[c - 1] > capraw - headroom:
            routes.append(cur)
            cur, load = [], 0
        cur.append(int(c))
        load += int(raw[c - 1])
    routes.append(cur)
    return routes


def flat(routes):
    return [x for r in routes for x in r + [0]]


def load_of(route, raw):
    return sum(int(raw[c - 1]) for c in route)


def overload(rng, routes, raw, capraw, target):
    """Move customers from the other routes (never emptying one) into route `target` until it carries more than the
    capacity; -> new routes, or None where the instance cannot overload it."""
    routes = [list(r) for r in routes]
    donors = [i for i in rng.permutation(len(routes)) if i != target % len(routes)]
    for i in donors:
        while len(routes[i]) > 1 and load_of(routes[target], raw) <= capraw:
            routes[target].append(routes[i].pop())
    return routes if load_of(routes[target], raw) > capraw else None


def first_over_step(tour, raw, capraw):
    load = 0
    for t, a in enumerate(tour):
        load = 0 if a == 0 else load + int(raw[a - 1])
        if load > capraw:
            return t
    return None


def cvrp_rows(rng, N, raw, capraw, n_valid, head=1):
    """-> list of (tour, class) for one instance with integer demands `raw` (demand = raw / capraw, capacity 1).
    head 1 keeps every load of a valid row a whole unit away from the capacity; 0 lets a route fill the vehicle."""
    rows = []
    for _ in range(n_valid):
        rows.append((flat(routes_for(rng, raw, capraw, head)), "valid"))
    base = routes_for(rng, raw, capraw, head)
    tour = flat(base)
    cust = [t for t, a in enumerate(tour) if a != 0]
    hi = max(tour)
    rows.append((tour + [hi], "twice"))                                    # the highest id once more, nobody missing
    rows.append((tour + [tour[cust[0]]], "twice"))
    for t in (cust[0], cust[-1], cust[len(cust) // 2]):
        rows.append((tour[:t] + [0] + tour[t + 1:], "missing"))
    rows.append(([0 if a == hi else a for a in tour], "missing"))
    for target, name in ((-1, "over_last"), (0, "over_first")):
        for _ in range(2):
            moved = overload(rng, routes_for(rng, raw, capraw, head), raw, capraw, target)
            if moved is None:
                continue
            tr = flat(moved)
            step = first_over_step(tr, raw, capraw)
            if target == -1:
                assert step >= len(tr) - len(moved[-1]) - 1
                rows.append((tr, "over_step64" if step >= 64 else "over_last"))
                if step >= 64:
                    rows.append((list(tr), "over_last"))
            else:
                assert step < len(moved[0])
                rows.append((tr, name))
    for i in range(len(base) - 1):
        if load_of(base[i], raw) + load_of(base[i + 1], raw) > capraw:
            rows.append((flat(base[:i] + [base[i] + base[i + 1]] + base[i + 2:]), "merge"))
            break
    return rows


def exact_cvrp_instance(rng, N):
    """Demands in units of 1/64, capacity 1: one route of `routes` loads to exactly 64/64, and a customer of demand 1/64
    in another route can be moved into it (65/64)."""
    raw = rng.integers(1, 17, size=N)
    if N == 3:
        return np.array([40, 24, 1]), [[1, 2], [3]]
    routes = routes_for(rng, raw, 64, 0)
    assert len(routes) >= 2
    full, other = routes[0], routes[1]
    raw[full[-1] - 1] += 64 - load_of(full, raw)
    raw[other[0] - 1] = 1
    assert load_of(full, raw) == 64 and load_of(other, raw) <= 64
    return raw, routes


def exact_cvrp_rows(raw, routes):
    rows = [(flat(routes), "exact_full"), (flat(routes[::-1]), "exact_full")]
    small = routes[1][0]
    moved = [routes[0] + [small]] + ([routes[1][1:]] if len(routes[1]) > 1 else []) + routes[2:]
    rows.append((flat(moved), "exact_over"))
    rows.append((flat(moved[::-1]), "exact_over"))
    return rows


def threshold_cvrp_instance(rng, N):
    """The capacity limit itself.  Customer 1 fills the vehicle (demand 1.0), customer 2 asks for 84 ULP, customer 3 for
    85 ULP, the others for k / 64.  1 and 2 in one route load it to exactly float32(1 + 1e-5), in either order: valid,
    since the reference asserts `used <= capacity + 1e-5`.  1 and 3 load it one ulp over.  That route comes first (the
    decisive step is 1), in the middle, or last (a step >= 64 from 64 customers on), each in both orders.
    -> (demand [N] float32, list of (tour, class))."""
    raw = rng.integers(1, 17, size=N - 3)
    demand = np.concatenate([[1.0, 84 * ULP, 85 * ULP], raw / 64.0]).astype(np.float32)
    assert demand[0] == 1.0 and float(demand[1]) == 84 * ULP and float(demand[2]) == 85 * ULP
    assert np.float32(1.0) + np.float32(1e-5) == np.float32(1.0) + demand[1]
    others = [[c + 3 for c in r] for r in routes_for(rng, raw, 64, 1)] if N > 3 else []
    rows = []
    for partner, lone, name in ((2, 3, "exact_at_limit"), (3, 2, "exact_ulp_over")):
        for pair in ([1, partner], [partner, 1]):
            for place in ("first", "middle", "last"):
                if place == "first":
                    routes = [pair] + others + [[lone]]
                elif place == "middle":
                    routes = others[:len(others) // 2] + [pair] + others[len(others) // 2:] + [[lone]]
                else:
                    routes = [[lone]] + others + [pair]
                rows.append((flat(routes), name))
    rows.append((flat([[2], [3]] + others + [[1]]), "valid"))
    return demand, rows


def pad_rows(rows, extra=1):
    T = max(len(r) for r, _ in rows) + extra
    return [(r + [0] * (T - len(r)), c) for r, c in rows]


# ---------------------------------------------------------------------------------------------------------
# the envs
# ---------------------------------------------------------------------------------------------------------
def build_tsp(rng):
    groups = []
    for N in NODES:
        g = Group()
        n_bad = 0
        perm = lambda: rng.permutation(N)
        for pos, name in ((0, "dup_pos0"), (63, "dup_pos63"), (64, "dup_pos64"), (N - 1, "dup_poslast")):
            if pos >= N:
                continue
            for _ in range(2):
                a = perm()
                a[pos] = a[(pos + 1 + rng.integers(N - 1)) % N]          # the node that was here is now missing
                g.add(0, a, name)
                n_bad += 1
        for node in (31, 32, 63, 64):
            if node >= N:
                continue
            a = perm()                                                     # `node` twice, another node missing
            t = int(rng.choice(np.flatnonzero(a != node)))
            a[t] = node
            g.add(0, a, f"dup_id{node}")
            a = perm()                                                     # `node` missing, its neighbour id twice
            a[np.flatnonzero(a == node)[0]] = node - 1 if node % 2 == 0 else node + 1 if node + 1 < N else node - 1
            g.add(0, a, f"dup_id{node}")
            n_bad += 2
        for _ in range(max(4, n_bad // 2)):
            g.add(0, perm(), "valid")
        groups.append(g)
    return groups


def build_cvrp(rng):
    groups = []
    for N in NODES:
        g = Group()
        rows_by_inst = []
        capraw = 12 if N == 3 else 30
        for _ in range(2):                                                 # demands k / 30: not representable
            raw = rng.integers(1, 10, size=N)
            b = g.add_instance(demand=(raw / capraw).astype(np.float32), capacity=np.float32(1.0))
            rows_by_inst.append((b, cvrp_rows(rng, N, raw, capraw, 6)))
        for _ in range(3):                                                 # demands k / 64: exact
            raw, routes = exact_cvrp_instance(rng, N)
            b = g.add_instance(demand=(raw / 64.0).astype(np.float32), capacity=np.float32(1.0))
            rows = cvrp_rows(rng, N, raw, 64, 3, head=0) + exact_cvrp_rows(raw, routes)
            rows_by_inst.append((b, rows))
        demand, rows = threshold_cvrp_instance(rng, N)
        rows_by_inst.append((g.add_instance(demand=demand, capacity=np.float32(1.0)), rows))
        allrows = pad_rows([rc for _, rows in rows_by_inst for rc in rows])
        it = iter(allrows)
        for b, rows in rows_by_inst:
            for _ in rows:
                r, c = next(it)
                g.add(b, r, c)
        groups.append(g)
    return groups


def sdvrp_tour(rng, raw, unit=1024, stop_after=None):
    """A feasible split-delivery tour by simulation: random customer order, deliver what fits, go back when full and
    come again for the rest.  Ends with one depot visit.  stop_after: cut after that many customers are fully served."""
    left = raw.astype(np.int64).copy()
    tour, used, done = [], 0, 0
    order = rng.permutation(len(raw)) + 1
    for c in order:
        while left[c - 1] > 0:
            if used == unit:
                tour.append(0)
                used = 0
            give = min(left[c - 1], unit - used)
            tour.append(int(c))
            left[c - 1] -= give
            used += give
        done += 1
        if stop_after is not None and done >= stop_after:
            return tour
    return tour + [0]


def build_sdvrp(rng):
    groups = []
    for N in NODES:
        g = Group()
        rows = []
        for k in range(4):
            light = k == 3                                                 # everything fits one vehicle: no depot needed
            raw = rng.integers(1, 4, size=N) if light else rng.integers(32, 700, size=N)
            b = g.add_instance(demand=(raw / 1024.0).astype(np.float32), capacity=np.float32(1.0))
            for _ in range(4):
                rows.append((b, sdvrp_tour(rng, raw), "valid", "revisit"))
            for _ in range(2):
                t = sdvrp_tour(rng, raw)
                p = int(rng.choice([i for i, a in enumerate(t) if a != 0]))      # the same customer again at once
                rows.append((b, t[:p + 1] + [t[p]] + t[p + 1:], "revisit_valid", "revisit"))
            for _ in range(2):
                rows.append((b, sdvrp_tour(rng, raw), "end_twice_valid", "zeros"))
                rows.append((b, [0, 0] + sdvrp_tour(rng, raw), "start_twice", "revisit"))
            if N > 1:
                for _ in range(2):
                    cut = sdvrp_tour(rng, raw, stop_after=int(rng.integers(1, N)))
                    rows.append((b, cut, "left", "revisit_open"))
                    rows.append((b, cut, "twice_and_left", "zeros"))
            if light:
                for _ in range(3):
                    rows.append((b, [int(c) for c in rng.permutation(N) + 1], "no_depot", "revisit_open"))
        T = max(len(r[1]) for r in rows) + 3
        for b, tour, cls, pad in rows:
            n = T - len(tour)
            if pad == "zeros":
                tour = tour + [0] * n
            elif pad == "revisit":                                         # come again to the last customer, then go home
                last = [a for a in tour if a != 0][-1]
                body = tour[:-1] if tour[-1] == 0 else tour
                tour = body + [last] * (T - len(body) - 1) + [0]
            else:                                                          # no closing depot visit either
                last = [a for a in tour if a != 0][-1]
                tour = tour + [last] * n
            g.add(b, tour, cls)
        groups.append(g)
    return groups


def build_pctsp(rng):
    groups = []
    for N in NODES:
        g = Group()
        rows = []

        def collect(prize, lo, hi=None):
            """Random customers until the float64 prize is >= lo (and, with hi, stays below hi)."""
            tour, total = [], 0.0
            for c in rng.permutation(N) + 1:
                if total >= lo:
                    break
                if hi is not None and total + float(prize[c]) >= hi:
                    continue
                tour.append(int(c))
                total += float(prize[c])
            return tour, total

        for k in range(2):                                                 # random float32 prizes, about 4 / N each (N >= 20)
            prize = np.zeros(N + 1, np.float32)
            prize[1:] = (rng.random(N) * (8.0 / max(N, 8)) + 0.01).astype(np.float32)
            if N == 3:
                prize[1:] = np.float32([0.55, 0.6, 0.3])
            b = g.add_instance(real_prize=prize)
            for _ in range(6):
                tour, total = collect(prize, 1.0 + 0.004)
                assert total >= 1.0 + 0.004
                rows.append((b, tour + [0], "valid"))
            for _ in range(3):
                tour, total = collect(prize, 0.7, hi=0.99)
                assert total < 0.99 and 0 < len(tour) < N
                rows.append((b, tour + [0], "short"))
            tour, _ = collect(prize, 1.0 + 0.004)
            rows.append((b, tour[:-1] + [tour[0], 0], "dup"))
            rows.append((b, tour + [0, tour[-1]], "dup"))
            rows.append((b, list(rng.permutation(N) + 1) + [N], "dup"))
            rows.append((b, [0, 0], "only_depot"))
        prize = np.zeros(N + 1, np.float32)                                # a poor instance: all prizes together 0.9
        w = rng.random(N) + 0.2
        prize[1:] = (0.9 * w / w.sum()).astype(np.float32)
        b = g.add_instance(real_prize=prize)
        for _ in range(5):
            rows.append((b, list(rng.permutation(N) + 1) + [0], "short_all_visited"))
        rows.append((b, list(rng.permutation(N) + 1), "short_all_visited"))
        if N > 1:
            rows.append((b, list(rng.permutation(N)[:N - 1] + 1) + [0], "short"))
        rows.append((b, [0], "only_depot"))
        for k in range(2):                                                 # prizes k / 64: exact
            raw = np.zeros(N + 1, np.int64)
            raw[1:] = rng.integers(1, 9, size=N) if N >= 20 else [30, 34, 33]
            b = g.add_instance(real_prize=(raw / 64.0).astype(np.float32))
            for want, name in ((64, "exact_one"), (63, "exact_short")):
                for _ in range(3):
                    for _try in range(1000):                               # fill greedily until the total is hit exactly
                        tour, total = [], 0
                        for c in rng.permutation(N) + 1:
                            if total + raw[c] <= want:
                                tour.append(int(c))
                                total += int(raw[c])
                        if total == want and len(tour) < N:
                            break
                    assert total == want and len(tour) < N, (N, total, want)
                    rows.append((b, tour + [0], name))
        padded = pad_rows([(r, c) for _, r, c in rows])
        for (b, _, _), (r, c) in zip(rows, padded):
            g.add(b, r, c)
        groups.append(g)
    return groups


def op_length(locs, tour):
    p = locs[np.array(tour + [0])].astype(np.float64)
    return float(np.sqrt(((np.roll(p, -1, axis=0) - p) ** 2).sum(-1)).sum())


def build_op(rng):
    groups = []
    for N in NODES:
        g = Group()
        rows = []
        for k in range(3):
            locs = rng.random((N + 1, 2)).astype(np.float32)
            L = np.float32((2.0, 3.0, 4.0)[k])
            d0 = vr._dist32(locs[0][None], locs)
            b = g.add_instance(locs=locs, max_length=(L - d0).astype(np.float32))

            def grow(lo, hi):
                """Random customers while the closed length stays below hi; accepted once it is in [lo, hi)."""
                for _ in range(200):
                    tour = []
                    for c in rng.permutation(N) + 1:
                        if op_length(locs, tour + [int(c)]) < hi:
                            tour.append(int(c))
                    if lo <= op_length(locs, tour) < hi and tour:
                        return tour
                return None

            for _ in range(5):
                tour = grow(0.0, float(L) - 0.01)
                if tour:
                    rows.append((b, tour + [0], "valid"))
            for _ in range(2):
                tour = grow(0.0, float(L) - 0.01)
                if tour and len(tour) >= 2:
                    cut = len(tour) // 2                                   # home in between: allowed
                    t2 = tour[:cut] + [0] + tour[cut:] + [0]
                    if op_length(locs, t2) < float(L) - 0.01:
                        rows.append((b, t2, "repeat_depot_valid"))
                    rows.append((b, tour[:-1] + [tour[0], 0], "dup"))
            tour = list(rng.permutation(N) + 1)
            rows.append((b, [int(c) for c in tour[:max(1, N // 2)]] + [0, int(tour[0])], "dup"))
            for _ in range(3):                                             # keep adding customers past the limit
                tour = []
                for c in rng.permutation(N) + 1:
                    tour.append(int(c))
                    if op_length(locs, tour) >= float(L) + 0.01:
                        break
                if op_length(locs, tour) >= float(L) + 0.01:
                    rows.append((b, tour + [0], "too_long"))
        padded = pad_rows([(r, c) for _, r, c in rows])
        for (b, _, _), (r, c) in zip(rows, padded):
            g.add(b, r, c)
        groups.append(g)
    return groups


def tailor_windows(rng, locs, dur, tour, mode, N):
    """Integer windows around the service starts of `tour` (simulated with the reference's rule).  mode: 'nowait' (every
    window is open on arrival), 'wait' (some open later), 'exact' (they close exactly at the start of service), or
    ('late', step): as 'nowait', but the customer at that step has a window that closed one unit before."""
    tw = np.zeros((N + 1, 2), np.int32)
    clock, node = 0.0, 0
    late_step = mode[1] if isinstance(mode, tuple) else None
    for t, a in enumerate(tour):
        if a == 0:
            clock, node = 0.0, 0
            continue
        d = float(np.sqrt(float(((locs[node] - locs[a]) ** 2).sum())))
        arrive = int(clock + d)
        if t == late_step:
            assert arrive >= 2
            tw[a] = (0, arrive - 1)
            start = arrive
        else:
            wait = mode == "wait" and rng.random() < 0.4
            start = arrive + (int(rng.integers(1, 6)) if wait else 0)
            ws = start if wait else max(0, arrive - int(rng.integers(0, 8)))
            we = start if mode == "exact" else start + int(rng.integers(1, 6))
            we = max(we, 1)
            if we <= ws:
                ws = we - 1
            assert ws >= 0
            tw[a] = (ws, we)
        clock, node = float(start) + float(dur[a]), a
    d0 = np.sqrt(((locs - locs[0]) ** 2).sum(-1))
    tw[0] = (0, int(np.ceil((tw[:, 0] + d0 + dur).max())) + 10)
    return tw


def build_cvrptw(rng):
    groups = []
    for N in NODES:
        g = Group()
        rows = []

        def instance(locs, raw, dur, tour, mode):
            tw = tailor_windows(rng, locs.astype(np.float64), dur, tour, mode, N)
            return g.add_instance(locs=locs.astype(np.float32), demand=(raw / 64.0).astype(np.float32),
                                  capacity=np.float32(1.0), time_windows=tw, durations=dur.astype(np.float32))

        for k in range(2):
            locs = rng.integers(0, 101, size=(N + 1, 2))
            raw = rng.integers(1, 17, size=N)
            dur = np.concatenate([[0], rng.integers(0, 12, size=N)])
            routes = routes_for(rng, raw, 64, 1)
            tour = flat(routes)
            b = instance(locs, raw, dur, tour, "nowait" if k == 0 else "wait")
            name = "valid" if k == 0 else "wait_valid"
            for _ in range(5):
                rows.append((b, tour, name))
            rows.append((b, tour[:-1] + [0, 0], name))
            # the CVRP part on this instance (the reference asserts it first)
            others = cvrp_rows(rng, N, raw, 64, 0)
            cust = [t for t, a in enumerate(tour) if a != 0]
            rows.append((b, tour + [tour[cust[-1]]], "twice"))
            rows.append((b, tour[:cust[0]] + [0] + tour[cust[0] + 1:], "missing"))
            rows += [(b, r, c) for r, c in others if c.startswith(("over", "merge"))]
            # late rows: the same tour on an instance whose window at one step closed one unit before the arrival
            resets = [t + 1 for t, a in enumerate(tour[:-1]) if a == 0]
            late = [("late_first", 0)]
            if resets:
                late.append(("late_after_reset", resets[-1]))
                late.append(("late_after_reset", resets[0]))
            if cust[-1] >= 64:
                late.append(("late_step64", cust[-1]))
                late.append(("late_step64", next(t for t in cust if t >= 64)))
            for cls, step in late:
                d = np.sqrt(float(((locs[tour[step - 1] if step else 0] - locs[tour[step]]) ** 2).sum()))
                if step in [0] + resets and int(d) < 2:
                    continue
                try:
                    rows.append((instance(locs, raw, dur, tour, ("late", step)), tour, cls))
                except AssertionError:
                    continue
        # 3-4-5 legs: every arrival is an integer exactly; the windows close exactly on arrival / one unit before
        n_path = min(N, 12)
        locs = rng.integers(0, 101, size=(N + 1, 2))
        locs[0] = (50, 50)
        p = np.array([50, 50])
        for i in range(1, n_path + 1):
            for _ in range(100):
                k = int(rng.integers(1, 4))
                step = np.array([(3, 4), (4, 3), (-3, 4), (4, -3), (-4, 3), (3, -4), (-3, -4), (-4, -3), (5, 0), (0, -5)][rng.integers(10)]) * k
                if ((p + step) >= 0).all() and ((p + step) <= 100).all():
                    break
            p = p + step
            locs[i] = p
        raw = rng.integers(1, 4, size=N)
        dur = np.concatenate([[0], rng.integers(0, 12, size=N)])
        rest = routes_for(rng, raw[n_path:], 64, 1) if N > n_path else []
        routes = [list(range(1, n_path + 1))] + [[c + n_path for c in r] for r in rest]
        tour = flat(routes)
        b = instance(locs, raw, dur, tour, "exact")
        for _ in range(3):
            rows.append((b, tour, "exact_end"))
        for step in sorted({0, n_path // 2, n_path - 1}):
            if step == 0 and int(np.sqrt(float(((locs[0] - locs[1]) ** 2).sum()))) < 2:
                continue
            rows.append((instance(locs, raw, dur, tour, ("late", step)), tour, "exact_one_late"))
        padded = pad_rows([(r, c) for _, r, c in rows])
        for (b, _, _), (r, c) in zip(rows, padded):
            g.add(b, r, c)
        groups.append(g)
    return groups


BUILDERS = {"tsp": build_tsp, "cvrp": build_cvrp, "sdvrp": build_sdvrp, "pctsp": build_pctsp, "op": build_op,
            "cvrptw": build_cvrptw}


def finish(env, group):
    """Group -> dict of arrays (without verdicts)."""
    R = len(group.rows)
    T = max(len(r) for _, r, _ in group.rows)
    assert all(len(r) == T for _, r, _ in group.rows), "rows of one group have one length"
    g = {k: np.stack([np.asarray(x) for x in v]) for k, v in group.inst.items()}
    g["actions"] = np.array([r for _, r, _ in group.rows], dtype=np.int64).reshape(R, T)
    g["inst"] = np.array([b for b, _, _ in group.rows], dtype=np.int64)
    g["cls"] = np.array([c for _, _, c in group.rows])
    g["exact"] = np.zeros(R, dtype=bool)
    return g


# ---------------------------------------------------------------------------------------------------------
# the reference, one row at a time
# ---------------------------------------------------------------------------------------------------------
def reference_verdicts(env, g):
    import _refshim

    _refshim.install()
    import torch
    from tensordict import TensorDict  # the stand-in

    from rl4co.envs.routing.cvrp.env import CVRPEnv
    from rl4co.envs.routing.cvrptw.env import CVRPTWEnv
    from rl4co.envs.routing.op.env import OPEnv
    from rl4co.envs.routing.pctsp.env import PCTSPEnv
    from rl4co.envs.routing.sdvrp.env import SDVRPEnv
    from rl4co.envs.routing.tsp.env import TSPEnv

    torch.set_num_threads(1)
    cls = {"tsp": TSPEnv, "cvrp": CVRPEnv, "sdvrp": SDVRPEnv, "pctsp": PCTSPEnv, "op": OPEnv, "cvrptw": CVRPTWEnv}[env]
    code = {msg: c for c, msg in vr.MESSAGE[env].items()}
    out = np.zeros(g["actions"].shape[0], dtype=np.int64)
    for r, a in enumerate(g["actions"]):
        b = int(g["inst"][r])
        src = {}
        for k in INSTANCE_KEYS[env]:
            v = torch.from_numpy(np.ascontiguousarray(g[k][b:b + 1]))
            src["vehicle_capacity" if k == "capacity" else k] = v.reshape(1, 1) if k == "capacity" else v
        if env == "pctsp":
            src["locs"] = torch.zeros(1, g["real_prize"].shape[1], 2)     # only its node count is read
        td = TensorDict(src, batch_size=[1])
        before = {k: v.clone() for k, v in src.items()}
        try:
            cls.check_solution_validity(td, torch.from_numpy(a[None].copy()))
        except AssertionError as e:
            hit = [c for msg, c in code.items() if str(e).startswith(msg)]
            assert len(hit) == 1, f"{env} row {r}: unexpected assertion {e!r}"
            out[r] = hit[0]
        assert all(torch.equal(before[k], src[k]) for k in src), "the reference modified the instance"
    return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def load_groups(path):
    """-> list of group dicts of a validity_<env>.npz or reward_<env>.npz (also used by the tests)."""
    with np.load(path) as z:
        n = int(z["groups"].reshape(-1)[0])
        groups = [{k[len(f"g{i}_"):]: z[k] for k in z.files if k.startswith(f"g{i}_")} for i in range(n)]
    for g in groups:
        for k in ("actions", "inst", "verdict"):
            if k in g:
                g[k] = g[k].astype(np.int64)
    return groups


def main():
    for s, env in enumerate(("tsp", "cvrp", "sdvrp", "pctsp", "op", "cvrptw")):
        rng = np.random.default_rng(20250917 + s)
        out = {}
        groups = [finish(env, grp) for grp in BUILDERS[env](rng)]
        total, valid = 0, 0
        for i, g in enumerate(groups):
            res = evaluate(env, g)
            g["exact"] = res.margin < MARGIN
            check_margins(env, g, res)
            g["verdict"] = reference_verdicts(env, g)
            diff = np.flatnonzero(g["verdict"] != res.verdict)
            assert diff.size == 0, (f"{env} group {i}: the restatement differs from the reference on rows {diff[:8].tolist()} "
                                    f"({g['cls'][diff[:8]].tolist()}): {res.verdict[diff[:8]].tolist()} vs "
                                    f"{g['verdict'][diff[:8]].tolist()}")
            total += g["verdict"].size
            valid += int((g["verdict"] == 0).sum())
            for k, v in g.items():
                if k == "actions":
                    v = v.astype(np.int16)
                elif k in ("inst", "verdict"):
                    v = v.astype(np.int16)
                out[f"g{i}_{k}"] = v
        out["groups"] = np.int64(len(groups))
        path = os.path.join(HERE, f"validity_{env}.npz")
        write_npz(path, out)
        labels = np.concatenate([g["cls"] for g in groups])
        missing = [c for c in CLASSES[env] if c not in labels]
        assert not missing, f"{env}: no row of class {missing}"
        shapes = [tuple(g["actions"].shape) for g in groups]
        print(f"validity_{env}: rows {total} valid {valid} ({100.0 * valid / total:.0f} %) shapes {shapes} "
              f"{os.path.getsize(path)} bytes", flush=True)
        assert valid * 4 >= total


if __name__ == "__main__":
    main()
