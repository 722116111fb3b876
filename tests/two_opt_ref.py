"""Test-side restatement of the TSP 2-opt local search (numpy, float32), written from its contract:

    repeat while the last sweep's delta < -1e-6 and sweeps < max_iterations (the first sweep always runs if max_iterations > 0):
        delta = 0; for i in 1..n-2, for j in i+1..n-1 (this order):
            prev = t[i-1]; next = t[(j+1) % n]; skip if prev == t[j] or next == t[i]
            change = ((d[prev, t[j]] + d[t[i], next]) - d[prev, t[i]]) - d[t[j], next]      # float32, this order
            if change < delta: (p, q, delta) = (i, j, change)                               # strict: first minimum wins
        if delta < -1e-6: reverse t[p..q]

A sweep is one float32 [n, n] change matrix; np.argmin returns the first occurrence in row-major order, which is the scan
order.  Distances from coordinates are the project's leg expression sqrtf(fmaf(dy, dy, dx*dx)).  The GPU tests compare the
kernel against this at sizes the recorded fixtures do not cover; test_host_local_search.py pins it to those fixtures.

`full_size_case` generates the seeded inputs of the full-size GPU comparisons on the CPU, so that the host test can check the
distance expression on exactly those coordinates.
"""
from __future__ import annotations

import numpy as np

THRESHOLD = np.float32(-1e-6)


def _fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the float64 product is exact, the float64 sum is rounded to odd so that the final
    rounding to float32 is the only one that counts."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                                    # exact error of the float64 sum
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def distance_matrix(locs):
    """locs [..., n, 2] float32 -> [..., n, n] float32, d[i][j] = sqrtf(fmaf(dy, dy, dx*dx)) of locs[i] - locs[j]."""
    locs = np.asarray(locs, dtype=np.float32)
    dx = locs[..., :, None, 0] - locs[..., None, :, 0]
    dy = locs[..., :, None, 1] - locs[..., None, :, 1]
    return np.sqrt(_fma32(dy, dy, dx * dx))


def sweep(d, t):
    """One best-improvement sweep, in place on t.  -> True if a segment was reversed."""
    n = t.shape[0]
    if n < 3:
        return False
    prev = np.roll(t, 1)                                               # t[i-1]
    nxt = np.roll(t, -1)                                               # t[(j+1) % n]
    change = ((d[prev[:, None], t[None, :]] + d[t[:, None], nxt[None, :]]) - d[prev, t][:, None]) - d[t, nxt][None, :]
    assert change.dtype == np.float32
    ok = np.triu(np.ones((n, n), dtype=bool), 1)
    ok[0, :] = False                                                   # 1 <= i < j
    ok &= (prev[:, None] != t[None, :]) & (nxt[None, :] != t[:, None])
    change = np.where(ok, change, np.float32(np.inf))
    flat = int(np.argmin(change))
    delta = change.reshape(-1)[flat]
    if not delta < 0:                                                  # nothing below the initial delta = 0
        return False
    if delta < THRESHOLD:
        p, q = divmod(flat, n)
        t[p:q + 1] = t[p:q + 1][::-1].copy()
        return True
    return False


def two_opt(d, tour, max_iterations=1000):
    """d [n, n] float32, tour [n] -> (improved tour int64 [n], sweeps run)."""
    d = np.asarray(d, dtype=np.float32)
    t = np.array(tour, dtype=np.int64)
    sweeps = 0
    while sweeps < max_iterations:
        moved = sweep(d, t)
        sweeps += 1
        if not moved:
            break
    return t, sweeps


def two_opt_batch(actions, locs=None, distances=None, max_iterations=1000):
    """-> (tours [B, n] int64, iters [B] int32)."""
    actions = np.asarray(actions)
    tours = np.empty(actions.shape, dtype=np.int64)
    iters = np.empty(actions.shape[0], dtype=np.int32)
    for b in range(actions.shape[0]):
        d = distance_matrix(locs[b]) if distances is None else distances[b]
        tours[b], iters[b] = two_opt(d, actions[b], max_iterations)
    return tours, iters


# name -> (rows, nodes, max_iterations): the seeded full-size inputs of tests/test_gpu_local_search.py
FULL_SIZE = {
    "tsp100": (1024, 100, 1000),
    "tsp20": (256, 20, 1000),
    "tsp200": (64, 200, 1000),
    "tsp1024_cap20": (8, 1024, 20),
}


def full_size_case(name):
    """-> (locs [B, n, 2] float32 in [0, 1), random permutations [B, n] int64, max_iterations), seeded by the name."""
    B, n, max_it = FULL_SIZE[name]
    rng = np.random.default_rng([7, B, n])
    locs = rng.random((B, n, 2), dtype=np.float32)
    perms = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int64)
    return locs, perms, max_it
