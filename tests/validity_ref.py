"""A plain numpy restatement of the six `check_solution_validity` methods of the reference, row by row, for the tests of
the validity kernels (tests/golden/make_golden_validity.py, test_host_validity.py, test_gpu_validity.py).

    tsp     rl4co/envs/routing/tsp/env.py:161-168        cvrp    rl4co/envs/routing/cvrp/env.py:157-185
    sdvrp   rl4co/envs/routing/sdvrp/env.py:137-159      pctsp   rl4co/envs/routing/pctsp/env.py:180-204
    op      rl4co/envs/routing/op/env.py:178-209         cvrptw  rl4co/envs/routing/cvrptw/env.py:180-214

Every function takes the instance arrays [B, ...] and action rows [R, T]; row r belongs to instance `inst[r]`, by default
r % B (the "(s b)" order of a multistart batch).  It returns a `Result` of three arrays:

    verdict  [R] int     0 = valid, otherwise the first assertion of the reference that fails for that row alone (the
                         constants below; the text is in MESSAGE)
    margin   [R] float64 how far the quantity that decided the row is from its threshold, computed in float64: for a valid
                         row the smallest slack, for a failing row the largest excess.  inf where integers decide.
    counters [R, K] int  what the row adds to the counters of the kernels (K = 2; CVRPTW: the two of the CVRP check, then
                         the one of the time replay)

The comparisons are made in the number formats of the reference: a float32 running load clamped at 0 against the float32
`capacity + 1e-5`; a float32 prize sum against 1 - 1e-5; the float32 OP limit ((max_length + distance to depot) + 1e-6)
+ 1e-5; the CVRPTW arrival time truncated to an integer before the max with the window start.  Sums are taken in step
order; the reference's torch sums may associate differently, which is why the fixtures keep every margin at 1e-3 or
more, or use numbers that float32 adds exactly.

Two things are set by include/eamrl.h, not by the reference (which would raise an IndexError, or has no counters):

  * a row with an id < 0 or above the highest node id is an invalid tour: verdict RANGE, counted in the first counter
    (and by the CVRPTW time replay in its own counter), never read through;
  * the first failing assertion ends a row: TSP, CVRP, PCTSP and OP count a row in at most one counter.  SDVRP replays
    every row to its end, so a row may be counted both for "depot twice" and for "demand left"; the CVRPTW time replay
    runs apart from the CVRP check, so a row may be counted by both.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

F = np.float32
VALID = 0
RANGE = 9                      # an id out of range (eamrl.h): first counter
INVALID_TOUR, OVER_CAPACITY, LATE = 1, 2, 3          # tsp, cvrp, cvrptw
DEPOT_TWICE, DEMAND_LEFT = 1, 2                      # sdvrp, in the order in which the reference asserts them
DUPLICATES, PRIZE_SHORT = 1, 2                       # pctsp
TOO_LONG = 2                                         # op (DUPLICATES = 1)

MESSAGE = {
    "tsp": {INVALID_TOUR: "Invalid tour"},
    "cvrp": {INVALID_TOUR: "Invalid tour", OVER_CAPACITY: "Used more than capacity"},
    "sdvrp": {DEPOT_TWICE: "Cannot visit depot twice if any nonzero demand", DEMAND_LEFT: "All demand must be satisfied"},
    "pctsp": {DUPLICATES: "Duplicates", PRIZE_SHORT: "Total prize does not satisfy min total prize"},
    "op": {DUPLICATES: "Duplicates", TOO_LONG: "Max length exceeded"},
    "cvrptw": {INVALID_TOUR: "Invalid tour", OVER_CAPACITY: "Used more than capacity",
               LATE: "vehicle cannot start service before deadline"},
}


class Result(NamedTuple):
    verdict: np.ndarray
    margin: np.ndarray
    counters: np.ndarray


def _inst(actions, B, inst):
    R = actions.shape[0]
    return np.arange(R) % B if inst is None else np.asarray(inst)


def _collect(rows, K=2):
    v = np.array([r[0] for r in rows], dtype=np.int64)
    m = np.array([r[1] for r in rows], dtype=np.float64)
    c = np.array([r[2] for r in rows], dtype=np.int64).reshape(len(rows), K)
    return Result(v, m, c)


def _out_of_range(a, top):
    return bool(((a < 0) | (a > top)).any())


def _first_counter(verdict):
    """The counters of the envs whose rows end at their first failing assertion."""
    return [int(verdict in (1, RANGE)), int(verdict == 2)]


# ---- TSP -------------------------------------------------------------------------------------------------------------
def tsp(actions, num_loc=None):
    """Sorted, a row must be 0 .. n-1."""
    actions = np.asarray(actions)
    n = actions.shape[1] if num_loc is None else num_loc
    rows = []
    for a in actions:
        if _out_of_range(a, n - 1):
            v = RANGE
        else:
            v = VALID if a.shape[0] == n and np.array_equal(np.sort(a), np.arange(n)) else INVALID_TOUR
        rows.append((v, np.inf, _first_counter(v)))
    return _collect(rows)


# ---- CVRP ------------------------------------------------------------------------------------------------------------
def _cvrp_row(dem, cap, a):
    N = dem.shape[0]
    if _out_of_range(a, N):
        return RANGE, np.inf
    s = np.sort(a)
    if a.shape[0] < N or not np.array_equal(s[a.shape[0] - N:], np.arange(1, N + 1)) or (s[:a.shape[0] - N] != 0).any():
        return INVALID_TOUR, np.inf
    cap = F(cap)
    lim = F(cap + F(1e-5))
    change = np.where(a == 0, -cap, dem[np.maximum(a, 1) - 1]).astype(F)
    used, used64, over, slack = F(0), 0.0, False, np.inf
    for x in change:
        used = F(used + x)
        used64 += float(x)
        if used < 0:
            used = F(0)
        if used64 < 0:
            used64 = 0.0
        over |= bool(used > lim)
        slack = min(slack, float(lim) - used64)            # most negative = the largest excess
    return (OVER_CAPACITY, -slack) if over else (VALID, slack)


def cvrp(demand, capacity, actions, inst=None):
    """demand [B, N] float32 (customers), capacity [B] float32, actions [R, T]."""
    demand, capacity, actions = np.asarray(demand, F), np.asarray(capacity, F).reshape(-1), np.asarray(actions)
    rows = []
    for a, b in zip(actions, _inst(actions, demand.shape[0], inst)):
        v, m = _cvrp_row(demand[b], capacity[b], a)
        rows.append((v, m, _first_counter(v)))
    return _collect(rows)


# ---- SDVRP -----------------------------------------------------------------------------------------------------------
def _sdvrp_row(dem, cap, a):
    """The delivery replay over (-capacity, demand...): every visit delivers min(what is left there, free capacity), the
    depot empties the vehicle.  The depot slot turns 0 at the first depot visit and stays -capacity without one."""
    N = dem.shape[0]
    cap = F(cap)
    d = np.concatenate([[-cap], dem]).astype(F)
    d64 = d.astype(np.float64)
    used, used64 = F(0), 0.0
    twice, twice_margin, ranged = False, np.inf, False
    prev = None
    for x in a:
        if x < 0 or x > N:
            ranged = True
            break
        if prev == 0 and x == 0 and (d != 0).any() and not twice:
            twice, twice_margin = True, float(np.abs(d64).max())
        give = min(d[x], F(cap - used))
        d[x] = F(d[x] - give)
        used = F(used + give)
        give64 = min(d64[x], float(cap) - used64)
        d64[x] -= give64
        used64 += give64
        if x == 0:
            used, used64 = F(0), 0.0
        prev = x
    left = bool((d != 0).any())
    counters = [int(left or ranged), int(twice)]
    if ranged:
        return RANGE, np.inf, counters
    if twice:
        return DEPOT_TWICE, twice_margin, counters
    rest = float(np.abs(d64).max())
    if left:
        return DEMAND_LEFT, rest, counters
    return VALID, (np.inf if rest == 0.0 else 0.0), counters


def sdvrp(demand, capacity, actions, inst=None):
    demand, capacity, actions = np.asarray(demand, F), np.asarray(capacity, F).reshape(-1), np.asarray(actions)
    rows = [_sdvrp_row(demand[b], capacity[b], a) for a, b in zip(actions, _inst(actions, demand.shape[0], inst))]
    return _collect(rows)


# ---- PCTSP -----------------------------------------------------------------------------------------------------------
def _has_duplicates(a):
    s = np.sort(a)
    return not bool(((s[1:] == 0) | (s[1:] > s[:-1])).all())


def _pctsp_row(prize, a):
    M = prize.shape[0]
    if _out_of_range(a, M - 1):
        return RANGE, np.inf
    if _has_duplicates(a):
        return DUPLICATES, np.inf
    if int((a != 0).sum()) == M - 1:                     # everyone visited: the prize does not matter
        return VALID, np.inf
    p = np.concatenate([[F(0)], prize[1:]]).astype(F)[a]         # the depot collects nothing
    total = F(0)
    for x in p:
        total = F(total + x)
    need = F(1.0 - 1e-5)
    gap = float(p.astype(np.float64).sum()) - float(need)
    return (VALID, gap) if total >= need else (PRIZE_SHORT, -gap)


def pctsp(real_prize, actions, inst=None):
    """real_prize [B, M] float32 with the depot slot first."""
    real_prize, actions = np.asarray(real_prize, F), np.asarray(actions)
    rows = []
    for a, b in zip(actions, _inst(actions, real_prize.shape[0], inst)):
        v, m = _pctsp_row(real_prize[b], a)
        rows.append((v, m, _first_counter(v)))
    return _collect(rows)


# ---- OP --------------------------------------------------------------------------------------------------------------
def _dist32(p, q):
    d = (p - q).astype(F)
    return np.sqrt(F(d[..., 0] * d[..., 0]) + F(d[..., 1] * d[..., 1]), dtype=F)


def _op_row(locs, maxlen, a):
    M = locs.shape[0]
    if _out_of_range(a, M - 1):
        return RANGE, np.inf
    if _has_duplicates(a):
        return DUPLICATES, np.inf
    pts = locs[a]
    legs = _dist32(np.roll(pts, -1, axis=0), pts)                # the closed tour over the actions
    length = F(0)
    for x in legs:
        length = F(length + x)
    lim = ((maxlen + _dist32(locs[0][None], locs)).astype(F) + F(1e-6)).astype(F) + F(1e-5)
    p64 = pts.astype(np.float64)
    length64 = float(np.sqrt(((np.roll(p64, -1, axis=0) - p64) ** 2).sum(-1)).sum())
    l64 = locs.astype(np.float64)
    lim64 = maxlen.astype(np.float64) + np.sqrt(((l64 - l64[0]) ** 2).sum(-1)) + 1e-6 + 1e-5
    slack = float((lim64 - length64).min())
    return (VALID, slack) if bool((length <= lim.astype(F)).all()) else (TOO_LONG, -slack)


def op(locs, max_length, actions, inst=None):
    """locs [B, M, 2], max_length [B, M] float32 (per node, the distance back to the depot already taken off)."""
    locs, max_length, actions = np.asarray(locs, F), np.asarray(max_length, F), np.asarray(actions)
    rows = []
    for a, b in zip(actions, _inst(actions, locs.shape[0], inst)):
        v, m = _op_row(locs[b], max_length[b], a)
        rows.append((v, m, _first_counter(v)))
    return _collect(rows)


# ---- CVRPTW ----------------------------------------------------------------------------------------------------------
def _time_row(locs, tw, dur, a):
    """-> (late, margin).  Arrival = int(clock + leg); service starts at max(arrival, window start) and must not be after
    the window end; the clock is then start + duration, and 0 at the depot.  With integer windows the comparison is one
    of integers, so the margin is how far an arrival is from the integer at which its truncation would change.  An
    arrival that is an integer in float64 is left out: the fixtures' instances lie on an integer grid with integer
    durations (asserted where the margin is checked), where such an arrival is exact in float32 as well."""
    M = locs.shape[0]
    clock, clock64, node, late, margin = F(0), 0.0, 0, False, np.inf
    l64 = locs.astype(np.float64)
    for x in a:
        if x < 0 or x >= M:
            return True, np.inf
        arrive = F(clock + _dist32(locs[node], locs[x]))
        arrive64 = clock64 + float(np.sqrt(((l64[node] - l64[x]) ** 2).sum()))
        frac = arrive64 - np.floor(arrive64)
        if frac != 0.0:
            margin = min(margin, frac, 1.0 - frac)
        start = max(int(arrive), int(tw[x, 0]))
        late |= bool(start > tw[x, 1])
        clock = F(F(start) + dur[x])
        clock64 = float(max(int(np.floor(arrive64)), int(tw[x, 0]))) + float(dur[x])
        node = x
        if x == 0:
            clock, clock64 = F(0), 0.0
    return late, margin


def cvrptw(locs, demand, capacity, time_windows, durations, actions, inst=None):
    """locs [B, M, 2] with the depot first, demand [B, M-1], time_windows [B, M, 2] (start, end), durations [B, M]."""
    locs, demand, capacity = np.asarray(locs, F), np.asarray(demand, F), np.asarray(capacity, F).reshape(-1)
    tw, dur, actions = np.asarray(time_windows), np.asarray(durations, F), np.asarray(actions)
    rows = []
    for a, b in zip(actions, _inst(actions, locs.shape[0], inst)):
        v, m = _cvrp_row(demand[b], capacity[b], a)
        late, tm = _time_row(locs[b], tw[b], dur[b], a)
        m = min(m, tm)                 # the third counter is the time replay's on every row, so its margin always counts
        if v == VALID and late:
            v = LATE
        rows.append((v, m, _first_counter(v) + [int(late)]))
    return _collect(rows, K=3)
