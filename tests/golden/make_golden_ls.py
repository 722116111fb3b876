#!/usr/bin/env python3
"""Golden vectors of the TSP 2-opt local search, produced by RUNNING THE REFERENCE's own `TSPEnv.local_search`
(rl4co/envs/routing/tsp/env.py:187-192 -> rl4co/envs/routing/tsp/local_search.py:17-79) in the build container:

    python tests/golden/make_golden_ls.py

The result tours come from `TSPEnv.local_search(td, actions, max_iterations=...)` itself.  It does not return how many
sweeps it ran, so the method is called row by row with a counting wrapper in place of the module's `two_opt_once`: with
`njit` as the identity the reference's own loop looks that name up at call time, and the number of calls is the number of
sweeps.  Nothing of the loop is restated here.

`numba` is absent, so `_refshim.install_numba()` makes `njit` the identity and the functions run as the numpy they are
written in: `delta` and `change` are numpy float32 scalars.  Real numba types `delta` as float64 (it unifies the literal
`0` with a float32).  The two agree: every value `delta` takes is a float32, comparisons of float32 values are exact in
either width, and -1e-6 rounds to the float32 nearest to it (-9.99999997e-07, above -1e-6), so no float32 lies between the
two thresholds.

Only data is stored: inputs, the reference's distance matrix (N <= 100; a CRC32 of its bytes above), result tours and
sweep counts.
"""
from __future__ import annotations

import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refshim  # noqa: E402

_refshim.install()
_refshim.install_numba()

import torch  # noqa: E402
from tensordict import TensorDict  # noqa: E402  (the stand-in)

from rl4co.envs.routing.tsp import local_search as ref_ls  # noqa: E402
from rl4co.envs.routing.tsp.env import TSPEnv  # noqa: E402
from rl4co.utils.ops import get_distance_matrix  # noqa: E402

torch.set_num_threads(1)


def reference_run(locs, distances, actions, max_iterations):
    """-> (tours [B, n] int64 from TSPEnv.local_search, sweeps [B] int32, the float32 matrix the reference searched on)."""
    B = actions.shape[0]
    calls = [0]
    once = ref_ls.two_opt_once

    def counting(*args, **kwargs):
        calls[0] += 1
        return once(*args, **kwargs)

    tours = np.empty_like(actions)
    sweeps = np.zeros(B, dtype=np.int32)
    before = actions.copy()
    ref_ls.two_opt_once = counting
    try:
        for b in range(B):
            src = {"locs": torch.from_numpy(locs[b:b + 1])}
            if distances is not None:
                src["distances"] = torch.from_numpy(distances[b:b + 1])
            calls[0] = 0
            out = TSPEnv.local_search(TensorDict(src, batch_size=[1]), torch.from_numpy(actions[b:b + 1]),
                                      max_iterations=max_iterations).numpy()
            assert out.dtype == np.int64 and out.shape == (1, actions.shape[1])
            tours[b], sweeps[b] = out[0], calls[0]
    finally:
        ref_ls.two_opt_once = once
    assert np.array_equal(actions, before), "the reference modified its input"
    dm = get_distance_matrix(torch.from_numpy(locs)).numpy() if distances is None else distances
    assert dm.dtype == np.float32
    return tours, sweeps, dm


def save(name, locs, actions, max_iterations, distances=None):
    tours, sweeps, dm = reference_run(locs, distances, actions, max_iterations)
    n = actions.shape[1]
    out = dict(locs=locs, actions=actions, max_iterations=np.int64(max_iterations), tours=tours, iters=sweeps,
               ref_distances_crc32=np.uint32(zlib.crc32(np.ascontiguousarray(dm).tobytes())))
    if distances is not None:
        out["distances"] = distances
    elif n <= 100:
        out["ref_distances"] = dm
    path = os.path.join(HERE, f"ls_{name}.npz")
    np.savez_compressed(path, **out)
    moved = int((tours != actions).any(axis=1).sum())
    print(f"ls_{name}: B={actions.shape[0]} n={n} max_iterations={max_iterations} sweeps={sweeps.tolist()} "
          f"rows changed={moved} ({os.path.getsize(path)} bytes)", flush=True)
    return tours, sweeps


def perms(rng, B, n):
    return np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int64)


def main():
    rng = np.random.default_rng(20240607)
    u = lambda B, n: rng.random((B, n, 2), dtype=np.float32)

    # random permutations, run to convergence
    for n, B in ((20, 8), (50, 4), (100, 3)):
        save(f"rand{n}", u(B, n), perms(rng, B, n), 1000)
    save("rand200", u(2, 200), perms(rng, 2, 200), 1000)
    # the iteration cap and the large-N path
    save("rand500_cap30", u(1, 500), perms(rng, 1, 500), 30)
    locs50, acts50 = u(4, 50), perms(rng, 4, 50)
    save("rand50_cap3", locs50, acts50, 3)
    # an already 2-optimal tour: one sweep, unchanged
    opt, _ = save("rand50_b", locs50, acts50, 1000)
    _, sw = save("optimal50", locs50, opt, 1000)
    assert (sw == 1).all()
    # ties: a 6 x 6 grid with spacing 1/8 -- many candidates have exactly the same change, the first in scan order wins
    g = (np.stack(np.meshgrid(np.arange(6), np.arange(6), indexing="ij"), -1).reshape(36, 2) / 8.0).astype(np.float32)
    save("tie36", np.broadcast_to(g, (3, 36, 2)).copy(), perms(rng, 3, 36), 1000)
    # td["distances"]: a random asymmetric matrix pins the row / column order of the four terms (the 2-opt delta is not the true
    # change of length there, so the loop need not converge: the cap is part of the case)
    save("asym30", u(3, 30), perms(rng, 3, 30), 50, distances=rng.random((3, 30, 30), dtype=np.float32))
    # the smallest graphs: n = 3 has the single pair (1, 2), whose change is rounding noise around 0
    save("n3", u(8, 3), perms(rng, 8, 3), 1000)
    save("n4", u(8, 4), perms(rng, 8, 4), 1000)


if __name__ == "__main__":
    main()
