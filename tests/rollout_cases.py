"""The cases of the rollout-arithmetic tests (tests/test_host_rollout_ref.py on the CPU, tests/test_gpu_rollout_arith.py on the
GPU): the table of (env, kind, M, S), seeded instances, synthetic decoder caches and noise, and `check`, the one function that
judges a rollout -- a kernel's on the GPU, the float32 restatement's (mutated or not) on the CPU -- against the float64
restatement (tests/rollout_ref.py).

Kinds.  The cache scales (K, Lp, query parts) are reeval_cases.SCALES:
    normal, clip0, temp0.5, temp2, tie    `normal`; clip 0 / temperature 0.5 / 2 / twin nodes
    peaked                                `peaked`: near one-hot attention, |u| of several units
    policy                                `policy`: |u| <= 0.6, the scale at which the header promises 1e-5
    saturated                             `peaked` with the Lp scale raised (SATURATED) until, on the float64 restatement's own greedy
                                          rollout, at least half of the live steps have two or more feasible nodes with u >= 9.5:
                                          d_tanhf is exactly 1 above 9, so those nodes tie at exactly `clip`
A `tie` case has twin nodes (TWINS, where they fit in M): the rows of K, V, Lp, Pa, Pb, every per-node feature of the instance
and the noise of the higher node are copies of the lower one's.

Bounds (none comes from the kernels):
    policy cases        log-probs within 1e-5, the contract of include/eamrl.h
    every other case    MARGIN (reeval_cases: 4) * RATIO[kind] * the max-abs error of the float32 restatement's selected log-probs
                        against the float64 ones on the same actions; the float32 restatement is run in its two summation
                        orders (the logits as a matrix product and node by node, rollout_ref.run) and the larger error counts
    full vectors        the per-step kernel's full [R, M] log-prob vector: the same with the error taken over the feasible
                        entries of the restatement's full vectors, no RATIO (`bound_full`)
    selection           the float64 key of the chosen node within twice the log-prob bound of the float64 maximum
"""
import functools
import zlib

import numpy as np
import torch

import reeval_cases
import rollout_ref as ref
from eam_rl4co_amd import env_spec

f32 = np.float32
E, B = ref.E, 3
MARGIN = reeval_cases.MARGIN
# Kernel error / float32-restatement error allowed on the log-probs, per kind.  1 unless a kernel is measured beyond it on the
# MI355X for a reason that is written down here.
RATIO = {}
ENVS = ("tsp", "cvrp", "sdvrp", "pctsp", "op", "cvrptw", "pdp")
KINDS = ("normal", "peaked", "policy", "clip0", "temp0.5", "temp2", "saturated", "tie")
MODES = ("greedy", "sampling")
TWINS = ((1, 2), (3, 4), (31, 32), (63, 64), (5, 69))      # + (M - 2, M - 1): see the module text of the GPU test
FULL_M = {"tsp": (2, 20, 33, 65, 100, 112, 113, 128, 129), "cvrp": (21, 65, 112, 113, 129)}
SAT_U = 9.5
FAR = 1 << 20
# (Lp scale, reseed) of the `saturated` cases: the scale is doubled from `peaked`'s 8 until the condition above holds; where no
# scale can do it (two nodes: both signs must be right at step 0 of all three instances) the generator's seed is advanced instead
SATURATED_DEFAULT = (64.0, 0)
SATURATED = {"tsp_saturated_M2_S1": (1024.0, 4), "tsp_saturated_M2_S4": (1024.0, 120), "tsp_saturated_M2_S17": (1024.0, 10)}


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _table():
    rows = []
    for env in ENVS:
        for M in ((20, 65) if env == "tsp" else (21, 65)):
            rows += [(env, "normal", M, S) for S in (1, 4)]
    for env in ("tsp", "cvrp"):
        rows += [(env, kind, M, S) for kind in KINDS for M in FULL_M[env] for S in (1, 4, 17)]
    rows += [("sdvrp", kind, M, S) for kind in ("normal", "peaked", "tie") for M in (21, 113) for S in (1, 4)]
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def name_of(env, kind, M, S):
    return f"{env}_{kind}_M{M}_S{S}"


TABLE = _table()
CASES = {name_of(*r): dict(name=name_of(*r), env=r[0], kind=r[1], M=r[2], S=r[3]) for r in TABLE}
NAMES = list(CASES)


def twins(c):
    """The twin pairs (lower, higher) of a case: those of TWINS that fit, and the last two nodes."""
    if c["kind"] != "tie":
        return ()
    M = c["M"]
    lo = 0 if c["env"] == "tsp" else 1              # (the depot has no twin)
    out = [p for p in TWINS if p[1] < M]
    last = (M - 2, M - 1)
    if last[0] >= lo and all(set(last).isdisjoint(p) for p in out):
        out.append(last)
    return tuple(out)


def clip_temp(c):
    return (0.0 if c["kind"] == "clip0" else 10.0), {"temp0.5": 0.5, "temp2": 2.0}.get(c["kind"], 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def instances(c):
    """B = 3 random instances in step_ref's batch format.  No instance can strand a row: every demand fits an empty vehicle,
    every CVRPTW window is still open on arrival from the depot at time 0 (legs < 1.42, windows end at 2 or later)."""
    env, M = c["env"], c["M"]
    rng = np.random.default_rng(_seed("instances", env, M))
    N = M - 1
    batch = {"env": env}
    if env == "tsp":
        batch["locs"] = rng.random((B, M, 2)).astype(f32)
    else:
        batch["depot"] = rng.random((B, 2)).astype(f32)
        batch["locs"] = rng.random((B, N, 2)).astype(f32)
    if env in ("cvrp", "sdvrp", "cvrptw"):
        batch["demand"] = rng.integers(1, 10, (B, N)).astype(f32) / f32(30 if M <= 33 else 50)
    if env == "cvrptw":
        start = rng.integers(0, 4, (B, M))
        tw = np.stack([start, start + rng.integers(2, 7, (B, M))], -1).astype(np.int32)
        tw[:, 0] = (0, FAR)
        batch["time_windows"] = tw
        dur = (rng.random((B, M)) * 0.5).astype(f32)
        dur[:, 0] = 0
        batch["durations"] = dur
    if env == "pctsp":
        batch["deterministic_prize"] = (rng.random((B, N)) * 4 / N).astype(f32)
        batch["stochastic_prize"] = (rng.random((B, N)) * 8 / N).astype(f32)
        batch["penalty"] = (rng.random((B, N)) * 0.1).astype(f32)
    if env == "op":
        batch["prize"] = rng.random((B, N)).astype(f32)
        batch["max_length"] = np.array([2.0, 2.5, 3.0], f32)
    shift = 0 if env == "tsp" else 1
    for lo, hi in twins(c):
        for k in ("locs", "demand", "deterministic_prize", "stochastic_prize", "penalty", "prize"):
            if k in batch:
                batch[k][:, hi - shift] = batch[k][:, lo - shift]
        for k in ("time_windows", "durations"):
            if k in batch:
                batch[k][:, hi] = batch[k][:, lo]
    return batch


def cache(c):
    """The synthetic decoder cache, float32 tensors at the scales of reeval_cases.operands: K, V, Lp, Pa [B, M, E], Pb (TSP),
    gctx [B, E], Cvec [NC, E] (None for PDP), dyn [3, E] (SDVRP)."""
    env, kind, M = c["env"], c["kind"], c["M"]
    scale = kind if kind in ("peaked", "policy") else "peaked" if kind == "saturated" else "normal"
    ks, ls, qs = reeval_cases.SCALES[scale]
    reseed = 0
    if kind == "saturated":
        ls, reseed = SATURATED.get(c["name"], SATURATED_DEFAULT)
    g = torch.Generator().manual_seed(_seed("cache", c["name"], reseed))

    def randn(*shape, s=1.0):
        return torch.randn(*shape, generator=g) * s

    NC = ref.N_STATE_COLS[env]
    out = dict(K=randn(B, M, E, s=ks), V=randn(B, M, E), Lp=randn(B, M, E, s=ls), Pa=randn(B, M, E, s=0.7 * qs),
               Pb=randn(B, M, E, s=0.5 * qs) if env == "tsp" else None, gctx=randn(B, E, s=0.5 * qs),
               Cvec=randn(NC, E, s=0.5) if NC else None,
               dyn=randn(3, E, s=0.5) * torch.tensor([1.0, 1.0, ls])[:, None] if env == "sdvrp" else None)
    for lo, hi in twins(c):
        for k in ("K", "V", "Lp", "Pa", "Pb"):
            if out[k] is not None:
                out[k][:, hi] = out[k][:, lo]
    return out


def t_max(c):
    return env_spec.max_steps(c["env"], c["M"])


def noise(c):
    """[R, t_max, M] Exp(1) draws, float32; twins share theirs."""
    g = torch.Generator().manual_seed(_seed("noise", c["name"]))
    q = torch.empty(B * c["S"], t_max(c), c["M"]).exponential_(generator=g).clamp_(min=1e-30)
    for lo, hi in twins(c):
        q[..., hi] = q[..., lo]
    return q


@functools.lru_cache(maxsize=8)
def operands(name):
    """-> (case, batch, cache, noise); computed once, read-only."""
    c = CASES[name]
    return c, instances(c), cache(c), noise(c)


# ---------------------------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------------------------
def saturated_steps(op, r64):
    """[R, T] int: the number of feasible nodes with u64 >= SAT_U before every step."""
    return (op["mask"] & (r64["u"] >= SAT_U)).sum(-1)


def check(name, mode, actions, logps, min_sat_share=0.25, noise=None):
    """Judges one finished rollout of case `name`: actions [R, T] int64 and logps [R, T] (the steps that were executed); `noise`
    where the sampling rollout did not draw from the case's own.
    -> dict(misses = list of text, one per failed check; figures = dict; op, r64 = the float64 run on these actions)."""
    c, batch, cch, q = operands(name)
    q = q if noise is None else noise
    clip, temp = clip_temp(c)
    actions = torch.as_tensor(np.asarray(actions), dtype=torch.int64)
    logps = torch.as_tensor(np.asarray(logps)).double()
    R, T = actions.shape
    misses, fig = [], {}
    op = ref.operands_of(cch, batch, actions.numpy(), c["S"], 0, clip, temp)
    out = dict(misses=misses, figures=fig, op=op, r64=None)
    if not bool(op["feasible"].all()):
        r, t = (int(x) for x in (~op["feasible"]).nonzero()[0])
        misses.append(f"infeasible action {int(actions[r, t])} of row {r} at step {t}")
        return out
    if not op["all_done"]:
        misses.append("rows are left unfinished")
    r64 = ref.run(op, torch.float64)
    out["r64"] = r64
    done, live = op["done"], ~op["done"]
    r32 = [ref.run(op, torch.float32, chunk=16, rowwise=w) for w in (False, True)]
    err32 = max(float((r["logp"].double() - r64["logp"]).abs().max()) for r in r32)
    full32 = max(float((r["logp_all"].double() - r64["logp_all"])[op["mask"]].abs().max()) for r in r32)
    policy = c["kind"] == "policy"
    bound = 1e-5 if policy else MARGIN * RATIO.get(c["kind"], 1.0) * err32
    err = float((logps - r64["logp"]).abs().max())
    fig.update(err=err, bound=bound, err32=err32, bound_full=1e-5 if policy else MARGIN * full32)
    if not err <= bound:
        misses.append(f"log-probs {err:.3e} from float64, bound {bound:.3e}")
    if done.any() and not bool((logps[done] == 0).all()):
        misses.append("a finished row has a log-prob other than 0")
    key = ref.keys64(r64, mode, q)
    gap = (key.max(-1).values - key.gather(-1, actions[..., None]).squeeze(-1))[live]
    fig["gap"] = float(gap.max()) if gap.numel() else 0.0
    if not fig["gap"] <= 2 * bound:
        misses.append(f"selection: the chosen key is {fig['gap']:.3e} below the float64 maximum, bound {2 * bound:.3e}")
    for lo, hi in twins(c):
        a = actions.numpy()
        first = lambda n: np.where((a == n).any(1), (a == n).argmax(1), T)
        bad = np.flatnonzero(~(first(lo) < first(hi)))
        if len(bad):
            misses.append(f"tie rule: node {hi} before its lower twin {lo} in row {int(bad[0])}")
    if mode == "greedy" and clip > 0:
        nsat = saturated_steps(op, r64)
        sat = op["mask"] & (r64["u"] >= SAT_U)
        lowest = torch.where(sat.any(-1), sat.int().argmax(-1), torch.full_like(actions, c["M"]))
        bad = ((actions > lowest) & live).nonzero()
        if len(bad):
            r, t = (int(x) for x in bad[0])
            misses.append(f"saturation rule: row {r} step {t} chose {int(actions[r, t])} above the saturated node {int(lowest[r, t])}")
        fig["sat_share"] = float(((nsat > 0) & live).sum()) / max(int(live.sum()), 1)
        if c["kind"] == "saturated" and not fig["sat_share"] >= min_sat_share:
            misses.append(f"only {fig['sat_share']:.2f} of the live steps have a saturated feasible node")
    return out


def saturated_share_of_reference(name):
    """The share of the live steps of the float64 restatement's own greedy rollout at which two or more feasible nodes have
    u64 >= SAT_U."""
    c, batch, cch, _ = operands(name)
    clip, temp = clip_temp(c)
    actions, _ = ref.rollout(cch, batch, c["S"], "greedy", None, torch.float64, clip, temp, t_max(c))
    op = ref.operands_of(cch, batch, actions.numpy(), c["S"], 0, clip, temp)
    live = ~op["done"]
    return float(((saturated_steps(op, ref.run(op)) >= 2) & live).sum()) / int(live.sum())
