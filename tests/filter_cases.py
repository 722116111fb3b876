"""Shared by test_host_filter.py and test_gpu_filter.py: the recorded filter cases (tests/golden/filter_cases.npz) and the
synthetic decoder caches that make a decode step produce a chosen row of scaled logits.

A cache is a dict of numpy arrays in the oracle's layout (K, V, Lp, Pa, Pb [B, M, E], cvec [E], gctx [B, E]) for a TSP
instance with E = 128, H = 8; with clip = 0 and temperature 1 the filter's input x is exactly the step's logits.

  * crafted rows: K = 0 makes every glimpse weight exp(0) = 1, V[n] = (1, 0, 0, ...) for every node makes the glimpse
    output exactly (1, 0, 0, ...), so node n's logit is float32(Lp[n][0] * c) with c = float32(1 / sqrt(128)), whatever
    the other (random) columns of Lp hold: equal Lp[n][0] give bit-identical logits (the ties), zero gives the uniform rows,
    and the row equals the recorded x bit for bit (the tests assert that before they compare verdicts);
  * random rows: everything random, Lp scaled so that the logits spread by about 0.1, 1 or 5; x is then whatever the
    implementation under test computed, and the restatement is applied to that.
"""
import os

import numpy as np

import filter_ref as fr

E, H = 128, 8
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_cases.npz")
INV_SQRT_E = np.float32(1.0) / np.sqrt(np.float32(E))
SIZES = (2, 5, 21, 64, 65, 101, 128, 129, 257)
TOP_P = (0.1, 0.5, 0.8, 0.95)
SCALES = (0.1, 1.0, 5.0)
MAX_SKIP_SHARE = 0.01


def top_ks(M):
    return (0, 3, M // 2)


def crafted_x(a):
    """The row a crafted cache produces from the column-0 values `a` of Lp (nan = masked node)."""
    a = np.asarray(a, np.float32)
    x = (np.nan_to_num(a) * INV_SQRT_E).astype(np.float32)
    x[np.isnan(a)] = -np.inf
    return x


def load_cases():
    """-> list of dicts: name, crafted, members, x, a, top_k, top_p, keep, logp (the reference's float32 log-probs)."""
    with np.load(PATH) as z:
        off = z["off"]
        return [dict(name=str(z["name"][i]), crafted=bool(z["crafted"][i]), members=bool(z["members"][i]),
                     top_k=int(z["top_k"][i]), top_p=float(z["top_p"][i]), x=z["x"][off[i]:off[i + 1]],
                     a=z["a"][off[i]:off[i + 1]], keep=z["keep"][off[i]:off[i + 1]], logp=z["logp"][off[i]:off[i + 1]])
                for i in range(off.size - 1)]


def crafted_cache(case, seed=0):
    """-> (cache, mask [1, M] u8) whose step logits are case["x"] exactly."""
    a = case["a"]
    M = a.size
    rng = np.random.default_rng(1000 + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    Lp = f(1, M, E)
    Lp[0, :, 0] = np.nan_to_num(a)
    V = np.zeros((1, M, E), np.float32)
    V[..., 0] = 1.0
    cache = {"K": np.zeros((1, M, E), np.float32), "V": V, "Lp": Lp, "Pa": f(1, M, E), "Pb": f(1, M, E), "cvec": f(E),
             "gctx": f(1, E)}
    return cache, (~np.isnan(a)).astype(np.uint8)[None]


def random_cache(M, seed):
    """-> (cache of B = 12 instances, mask [12, M] u8): four instances per logit scale, every second one with about a fifth
    of its nodes masked at random places (never all of them)."""
    B = 4 * len(SCALES)
    rng = np.random.default_rng(2000 + 7 * M + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    # the glimpse output is a convex combination of V rows, of norm about sqrt(E) / sqrt(nodes that carry weight); a
    # logit is its dot product with an Lp row / sqrt(E).  Normalising V rows makes the spread of the logits about `scale`.
    V = f(B, M, E)
    V /= np.linalg.norm(V, axis=-1, keepdims=True) / np.sqrt(E)
    Lp = f(B, M, E) * np.repeat(np.asarray(SCALES, np.float32), 4)[:, None, None] * np.float32(np.sqrt(min(M, 8.0)))
    cache = {"K": f(B, M, E) * np.float32(0.5), "V": V, "Lp": Lp, "Pa": f(B, M, E), "Pb": f(B, M, E), "cvec": f(E),
             "gctx": f(B, E)}
    mask = np.ones((B, M), np.uint8)
    for b in range(1, B, 2):
        drop = rng.random(M) < 0.2
        drop[rng.integers(M)] = False
        mask[b, drop] = 0
    return cache, mask


def check_keep(case, keep, what):
    """A crafted row's keep set against the recorded verdict: the same members where the reference's own sort kept the
    stable order, else the same number of members lost by every tie group."""
    if case["members"]:
        assert np.array_equal(keep, case["keep"]), (what, case["name"], np.flatnonzero(keep != case["keep"]).tolist())
    else:
        assert fr.removed_per_group(case["x"], keep) == fr.removed_per_group(case["x"], case["keep"]), (what, case["name"])
        assert not keep[~np.isfinite(case["x"])].any()


def check_logp(logp, keep, x, tol, what):
    """Log-probs of the kept entries against the float64 log-softmax of x over that keep set; -inf elsewhere."""
    z = x[keep].astype(np.float64)
    ref = z - z.max() - np.log(np.exp(z - z.max()).sum())
    err = float(np.abs(np.asarray(logp, np.float64)[keep] - ref).max())
    assert err <= tol, (what, err)
    assert np.isneginf(np.asarray(logp)[~keep]).all(), what
    return err
