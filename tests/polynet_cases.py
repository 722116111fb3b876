"""The cases of the PolyNet rollout-arithmetic tests (tests/test_host_polynet_arith.py on the CPU, tests/test_gpu_polynet_arith.py
on the GPU): the PolyNet case of the start-sharing rollout kernel (k_rollout_ms_mfma<..., PolyArgs>) against the float64
restatement of the PolyNet pointer (tests/rollout_ref.py, `poly`).

Everything but the pointer is tests/rollout_cases.py's, used through `as_rollout_case` (that module's generators run with this
module's case, batch size and ratio table for the duration of a call; the module is left as it was): instances, caches, noise,
the scales of reeval_cases.SCALES, `clip_temp`, TWINS and `check`.  Added per case: the unfolded logit key L [B, M, E] at the
scale of Lp (Lp becomes its fold L Wout, which no PolyNet kernel may read), the twins' rows of L in a `tie` case, and the
pointer's weights from a seeded generator:
    Wout   randn / sqrt(E)                 |g| is |heads|: with the residual below |u| stays at the scale of the kind
    W1     [randn / sqrt(E) | 0.5 randn]   the strategy columns move a hidden unit by about half a unit per bit
    b1     0.5 randn                       centred: about half of the hidden units are positive (checked: 20 % .. 80 %)
    W2     0.5 randn / sqrt(P),  b2  0.05 randn        the residual is a fraction of g
    Z      polynet_ref.binary_vectors(k)
The weight seed of a case is walked on the CPU (`walk_seed`) until the case's conditions hold and recorded in SEEDS; the L scale
of a `saturated` case is doubled from `peaked`'s 8 until at least half of the live steps of the float64 restatement's own
greedy rollout have two or more feasible nodes with u >= 9.5, and recorded in SATURATED.  tests/test_host_polynet_arith.py
re-checks every case.

Shapes (S rows per instance, B instances, k strategies), the smallest at which each path of the launcher can go wrong:
    min      2, 3, 2          the minimum                          uneven   40, 100, 16     three query tiles over two workgroups
    tile     16, 3, 16        one full query tile                  looped   17, 129, 2      nsplit = 1: two tiles looped in a workgroup
    tile+1   17, 3, 5         a second tile with one live query;   wide     128, 1, 128     eight workgroups per instance
                              k divides neither 16 nor 128         split    130, 3, 5       two launches: s_offset in the strategy and
    k1       4, 3, 1          an empty strategy vector                                      the noise row (k = 5: 128 % k != 0)
    k>S      2, 3, 5          more strategies than rows
`policy` and `normal` run on every M (every side of the key-tile switches 32 | 33 and 64 | 65, two nodes, the last size 112); the
other kinds on one M per tile count and env (20 / 21, 33, 65) in the shape tile+1, `tie` also at 112, where all of TWINS fit.
The large shapes run at M = 20 / 21: R T M^2 stays small enough for the float64 run of a case to take seconds; `uneven` and
`looped` on TSP only (the query-tile split does not depend on the env, and step_ref's CVRP replay of 4000 rows takes 13 s).

The CVRP `split` case decides whether the final state of a split rollout is padded against the final step count: its sampling
noise makes the rows of the last two starts prefer the depot (their depot draws are 1e-6: +13.8 on the depot's key), so they
return after every customer and need more steps than any row of the first 128 starts (confirmed on the CPU by the host test).

Bounds (none comes from the kernel): `policy` 1e-5, the contract of include/eamrl.h; every other kind rollout_cases.MARGIN (4) *
RATIO[kind] * the float32 restatement's own max-abs error against float64 on the same actions, the larger of its two
summation orders.  Selection, twins and the lowest saturated index as in rollout_cases.check.
"""
import contextlib
import zlib
from unittest import mock

import numpy as np
import torch

import polynet_ref
import rollout_cases as rc
import rollout_ref as ref

E, P = ref.E, 256
MARGIN = rc.MARGIN
# Kernel error / float32-restatement error allowed on the log-probs, per kind.  1 unless the kernel is measured beyond it on the
# MI355X for a reason that is written down here, with the measured figure.
RATIO = {}
KINDS = rc.KINDS
MODES = rc.MODES
SHAPES = {"min": (2, 3, 2), "tile": (16, 3, 16), "tile+1": (17, 3, 5), "k1": (4, 3, 1), "k>S": (2, 3, 5),
          "uneven": (40, 100, 16), "looped": (17, 129, 2), "wide": (128, 1, 128), "split": (130, 3, 5)}
# M -> the shapes of its `policy` and its `normal` case
EVERY_M = {"tsp": {2: ("min", "tile+1"), 20: ("tile+1", "tile"), 31: ("tile", "tile+1"), 32: ("tile+1", "min"), 33: ("k1", "tile+1"),
                   63: ("tile+1", "tile"), 64: ("tile", "k>S"), 65: ("k>S", "tile+1"), 100: ("min", "k1"), 112: ("tile+1", "min")},
           "cvrp": {21: ("tile+1", "tile"), 32: ("tile", "tile+1"), 33: ("min", "k1"), 64: ("tile+1", "k>S"), 65: ("k1", "tile+1"),
                    112: ("tile", "tile+1")}}
KIND_M = {"tsp": (20, 33, 65), "cvrp": (21, 33, 65)}
LARGE = ("uneven", "looped", "wide", "split")
DEPOT_DRAW = 1e-6           # the depot's noise of the last two starts of the CVRP `split` case


def name_of(env, kind, M, S, B, k):
    return f"{env}_{kind}_M{M}_S{S}_B{B}_k{k}"


def _table():
    rows = []
    for env, per_m in EVERY_M.items():
        for M, (pol, nor) in per_m.items():
            rows += [(env, "policy", M) + SHAPES[pol], (env, "normal", M) + SHAPES[nor]]
        for kind in KINDS:
            if kind not in ("policy", "normal"):
                rows += [(env, kind, M) + SHAPES["tile+1"] for M in KIND_M[env] + ((112,) if kind == "tie" else ())]
        rows += [(env, "normal", KIND_M[env][0]) + SHAPES[s] for s in LARGE[0 if env == "tsp" else 2:]]
    assert len(rows) == len(set(rows))
    return rows


TABLE = _table()
CASES = {name_of(*r): dict(name=name_of(*r), env=r[0], kind=r[1], M=r[2], S=r[3], B=r[4], k=r[5]) for r in TABLE}
NAMES = list(CASES)
SPLIT = [n for n in NAMES if CASES[n]["S"] > 128]
# one case per key-tile count (2, 4, 7 tiles) for the checks that run on a few cases only
PER_TILE_COUNT = ["tsp_normal_M20_S16_B3_k16", "tsp_normal_M33_S17_B3_k5", "tsp_normal_M65_S17_B3_k5", "cvrp_normal_M21_S16_B3_k16",
                  "cvrp_policy_M64_S17_B3_k5", "cvrp_normal_M112_S17_B3_k5"]
# weight seeds found by walk_seed (the first seed from 0 that meets the case's conditions); the cases not listed: 0
SEEDS = {}
# L scale of the `saturated` cases (doubled from `peaked`'s 8 until the condition of the module text holds); not listed: the default
SATURATED_DEFAULT = 64.0
SATURATED = {}


_rc_cache, _rc_noise = rc.cache, rc.noise


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


@contextlib.contextmanager
def as_rollout_case(c):
    """rollout_cases' generators and `check` see this module's case `c`, its batch size and this module's RATIO."""
    with mock.patch.dict(rc.CASES, {c["name"]: c}), mock.patch.object(rc, "B", c["B"]), mock.patch.object(rc, "RATIO", RATIO), \
            mock.patch.object(rc, "cache", cache), mock.patch.object(rc, "noise", noise):
        yield


def weights(c, seed):
    """The pointer's parameters in the reference's shapes, float32 (module text)."""
    k = c["k"]
    Z = torch.from_numpy(polynet_ref.binary_vectors(k))
    g = torch.Generator().manual_seed(_seed("polynet weights", c["name"], seed))
    randn = lambda *shape: torch.randn(*shape, generator=g)
    W1 = torch.cat([randn(P, E) / E ** 0.5, 0.5 * randn(P, Z.shape[1])], 1)
    return dict(Wout=randn(E, E) / E ** 0.5, W1=W1, b1=0.5 * randn(P), W2=0.5 * randn(E, P) / P ** 0.5, b2=0.05 * randn(E), Z=Z)


def cache(c, seed=None, l_scale=None):
    """rollout_cases.cache(c) plus L, Lp = its fold, and `poly`."""
    out = _rc_cache(dict(c, kind="peaked") if c["kind"] == "saturated" else c)
    scale = "peaked" if c["kind"] in ("peaked", "saturated") else "policy" if c["kind"] == "policy" else "normal"
    ls = rc.reeval_cases.SCALES[scale][1]
    if c["kind"] == "saturated":
        ls = SATURATED.get(c["name"], SATURATED_DEFAULT) if l_scale is None else l_scale
    g = torch.Generator().manual_seed(_seed("polynet L", c["name"]))
    L = torch.randn(c["B"], c["M"], E, generator=g) * ls
    for lo, hi in rc.twins(c):
        L[:, hi] = L[:, lo]
    poly = weights(c, SEEDS.get(c["name"], 0) if seed is None else seed)
    out.update(L=L, Lp=(L.double() @ poly["Wout"].double()).float(), poly=poly)
    return out


def noise(c):
    """rollout_cases.noise(c); the CVRP `split` case: module text."""
    q = _rc_noise(c)
    if c["env"] == "cvrp" and c["S"] > 128:
        q[128 * c["B"]:, :, 0] = DEPOT_DRAW
    return q


def t_max(c):
    return rc.t_max(c)


def clip_temp(c):
    return rc.clip_temp(c)


def operands(name):
    """-> (case, batch, cache, noise) of rollout_cases' generators for this module's case; read-only."""
    with as_rollout_case(CASES[name]):
        return rc.operands(name)


def operands_with(name, seed, l_scale=None):
    """`operands` with another weight seed / L scale (the walks below)."""
    c = CASES[name]
    with as_rollout_case(c):
        return c, rc.instances(c), cache(c, seed, l_scale), noise(c)


def check(name, mode, actions, logps, **kw):
    """rollout_cases.check on this module's case."""
    with as_rollout_case(CASES[name]):
        return rc.check(name, mode, actions, logps, **kw)


def polynet_operands(c, cch, device):
    """ops.polynet_operands of the case's weights, on `device`."""
    from eam_rl4co_amd import ops

    p = cch["poly"]
    return {k: (v.to(device) if torch.is_tensor(v) else v)
            for k, v in ops.polynet_operands(p["Wout"], p["W1"], p["b1"], p["W2"], p["b2"], p["Z"]).items()}


# ---------------------------------------------------------------------------------------------------------------------
# the conditions a case must meet
# ---------------------------------------------------------------------------------------------------------------------
def reference_rollout(c, batch, cch, q, mode="greedy", dtype=torch.float64):
    clip, temp = rc.clip_temp(c)
    return ref.rollout(cch, batch, c["S"], mode, q, dtype, clip, temp, rc.t_max(c))


def strategy_gap(c, op, r64):
    """The smallest over the instances of the largest max-abs difference between two strategies' full log-prob vectors at the
    first decision (float64)."""
    lp, mask = r64["logp_all"][:, 0], op["mask"][:, 0]
    B, S, k = c["B"], c["S"], c["k"]
    worst = np.inf
    for b in range(B):
        rows = [s * B + b for s in range(min(S, k))]
        assert bool((mask[rows] == mask[rows[0]]).all())
        v = lp[rows][:, mask[rows[0]]]
        worst = min(worst, float((v[:, None] - v[None]).abs().amax()))
    return worst


def relu_share(op, r64):
    """The share of positive hidden units over the live steps of a float64 run."""
    return float((r64["pre"][~op["done"]] > 0).double().mean())


def conditions(c, batch, cch, q):
    """-> (dict of figures, list of the conditions that fail) on the float64 restatement's own greedy rollout."""
    clip, temp = rc.clip_temp(c)
    actions, _ = reference_rollout(c, batch, cch, q)
    op = ref.operands_of(cch, batch, actions.numpy(), c["S"], 0, clip, temp)
    r64 = ref.run(op)
    r32 = [ref.run(op, torch.float32, chunk=16, rowwise=w) for w in (False, True)]
    err32 = max(float((r["logp"].double() - r64["logp"]).abs().max()) for r in r32)
    bound = 1e-5 if c["kind"] == "policy" else MARGIN * RATIO.get(c["kind"], 1.0) * err32
    fig = dict(bound=bound, relu=relu_share(op, r64), gap=strategy_gap(c, op, r64) if c["k"] > 1 else None,
               u=float(r64["u"][op["mask"] & ~op["done"][..., None]].abs().max()))
    fails = []
    if not 0.2 <= fig["relu"] <= 0.8:
        fails.append(f"{fig['relu']:.2f} of the hidden units are positive")
    if c["k"] > 1 and not fig["gap"] > 100 * bound:
        fails.append(f"the strategies of an instance are {fig['gap']:.3e} apart, 100 bounds are {100 * bound:.3e}")
    if c["kind"] == "saturated":
        live = ~op["done"]
        fig["sat"] = float(((rc.saturated_steps(op, r64) >= 2) & live).sum()) / int(live.sum())
        if not fig["sat"] >= 0.5:
            fails.append(f"only {fig['sat']:.2f} of the live steps have two saturated feasible nodes")
    return fig, fails


def walk_seed(name, limit=50, scales=(64.0, 128.0, 256.0, 512.0, 1024.0)):
    """-> (weight seed, L scale or None): the first that meet the conditions, the seed walked inside each L scale."""
    c = CASES[name]
    for ls in (scales if c["kind"] == "saturated" else (None,)):
        for seed in range(limit):
            _, batch, cch, q = operands_with(name, seed, ls)
            if not conditions(c, batch, cch, q)[1]:
                return seed, ls
    raise AssertionError(f"{name}: no weight seed below {limit} meets the conditions")


if __name__ == "__main__":          # python tests/polynet_cases.py: what to record in SEEDS and SATURATED
    found = {n: walk_seed(n) for n in NAMES}
    print("SEEDS =", {n: s for n, (s, _) in found.items() if s})
    print("SATURATED =", {n: ls for n, (_, ls) in found.items() if ls not in (None, SATURATED_DEFAULT)})
