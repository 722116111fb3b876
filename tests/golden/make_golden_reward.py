#!/usr/bin/env python3
"""Fixtures for the reward and log-likelihood kernels, with values recorded by RUNNING THE REFERENCE's own `_get_reward`
(tsp/env.py:152-158, cvrp/env.py:146-155, pdp/env.py:194-204, pctsp/env.py:158-178, op/env.py:166-175) and
`rl4co.utils.decoding.get_log_likelihood(logp, return_sum=True)` on the CPU, in the build container:

    python tests/golden/make_golden_reward.py

Rows are valid tours built here in numpy (validity is the subject of make_golden_validity.py, not of this file), placed
on purpose where the kernels can go wrong: leg counts P (T for TSP, T + 1 with a depot) and step counts T on both sides
of 64 and 128, rows that end at a customer (a long closing leg), at the depot, or in k depot visits of padding, and at
least 3 instances per group with the rows interleaved over them.

Two kinds of group per shape:
  exact    coordinates are distinct multiples of 1/1024 along x with y constant (`exact_x`) or along y (`exact_y`),
           penalties and prizes multiples of 1/64, log-probs multiples of 2^-10 in (-8, 0]: every leg and every partial
           sum is exact in float32 in any order.  The recorded value must equal the float64 value of tests/reward_ref.py
           bit for bit, or this script fails.
  generic  uniform float32 numbers.  A row is redrawn until the legs at steps 0, 63, 64, 127, 128, the last leg and the
           closing leg (and the prizes, penalties and log-probs at those steps) are at least max(0.05, 6 tol(row)), so
           that a dropped term moves the row by more than the derived tolerance (test_host_reward.py: the mutants).

One `reward_<env>.npz` per env (tsp, cvrp, pdp, pctsp, op, and `logp` for the log-prob rows) holds groups g0, g1, ... of one
shape each: `gK_actions` [R, T] int16, `gK_inst` [R], `gK_cls`, `gK_reward` [R] float32 as recorded, `gK_kind`, and the
instance arrays [B, ...].  PCTSP and OP also record the reference's `T == 1` special case (`t1_*`).  Only data is stored,
with fixed time stamps, so a rerun gives the same bytes.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import reward_ref as rr  # noqa: E402
from make_golden_validity import load_groups, write_npz  # noqa: E402,F401  (load_groups: for the tests)

ENVS = ("tsp", "cvrp", "pdp", "pctsp", "op", "logp")
# The reference has ONE reward per family: SDVRPEnv subclasses CVRPEnv and inherits `_get_reward` (sdvrp/env.py:17),
# CVRPTWEnv's only calls super()'s (cvrptw/env.py:163-166), SPCTSPEnv subclasses PCTSPEnv (spctsp/env.py:8) and the
# reward reads `penalty` alone.  They are recorded once, under the env on the right.
SHARED = {"sdvrp": "cvrp", "cvrptw": "cvrp", "spctsp": "pctsp"}
INSTANCE_KEYS = {"tsp": ("locs",), "cvrp": ("locs",), "pdp": ("locs",), "pctsp": ("locs", "penalty"), "op": ("prize",),
                 "logp": ()}
KINDS = ("exact_x", "exact_y", "generic")
EDGE = (63, 64, 65, 128, 129)                  # every env holds each of these as a leg count P and as a step count T
TSP_NODES = (2, 20, 62, 63, 64, 65, 127, 128, 129, 300)
# (customers N, steps T); with a depot P = T + 1
DEPOT_SHAPES = ((1, 2), (20, 24), (62, 62), (62, 63), (63, 64), (64, 65), (65, 70), (127, 127), (127, 128), (128, 129),
                (129, 135), (300, 310))
PDP_SHAPES = ((2, 2), (20, 20), (62, 62), (62, 63), (64, 64), (64, 65), (126, 127), (128, 128), (128, 129), (300, 300))
LOGP_STEPS = (1, 2, 20, 62, 63, 64, 65, 127, 128, 129, 300)
CLASSES = {"tsp": ("perm", "closing_long", "first_long"),
           "cvrp": ("ends_at_customer", "ends_at_depot", "pad_k"),
           "pdp": ("from_pickup", "depot_start", "ends_at_depot"),
           "pctsp": ("ends_at_customer", "ends_at_depot", "pad_k", "only_depot"),
           "op": ("ends_at_customer", "ends_at_depot", "pad_k", "only_depot"),
           "logp": ("logp", "zero_tail")}
B, ROWS = 3, 9
FLOOR, FLOOR_TOLS = 0.05, 6.0
EDGE_STEPS = (0, 63, 64, 127, 128)
T1_MESSAGE = "If all length 1 tours, they should be zero"


def evaluate(env, g, actions=None, inst="own", mutant=None):
    """reward_ref on the rows of a group."""
    a = g["actions"] if actions is None else actions
    i = g["inst"] if isinstance(inst, str) else inst
    if env == "logp":
        return rr.loglik(g["logp"] if actions is None else actions, mutant)
    if env == "pctsp":
        return rr.pctsp(g["locs"], g["penalty"], a, i, mutant)
    if env == "op":
        return rr.op(g["prize"], a, i, mutant)
    return rr.tour(g["locs"], a, i, env != "tsp", mutant)


def used_fraction(got, res):
    """The largest |got - float64| / tol over the rows; asserts that none exceeds 1 (a row without terms must be 0)."""
    diff, t = np.abs(np.asarray(got, np.float64) - res.value), rr.tol(res)
    assert (diff <= t).all(), f"rows {np.flatnonzero(diff > t)[:8].tolist()} are more than tol away from float64"
    return float((diff[t > 0] / t[t > 0]).max()) if (t > 0).any() else 0.0


def leg_count(env, g):
    return g["actions"].shape[1] + (env not in ("tsp", "logp"))


# ---------------------------------------------------------------------------------------------------------
# instances
# ---------------------------------------------------------------------------------------------------------
def make_locs(rng, kind, M):
    if kind == "generic":
        return rng.random((M, 2), dtype=np.float32)
    line = (rng.choice(1024, size=M, replace=False) / 1024.0).astype(np.float32)
    const = np.full(M, rng.integers(0, 1024) / 1024.0, np.float32)
    return np.stack([line, const] if kind == "exact_x" else [const, line], axis=1)


def make_node_values(rng, kind, M, scale):
    """Penalties (scale 0.25) or prizes (scale 1) with a zero depot slot; the last node's is kept away from zero."""
    v = np.zeros(M, np.float32)
    if kind == "generic":
        v[1:] = rng.random(M - 1, dtype=np.float32) * np.float32(scale)
        v[M - 1] = np.float32(scale * (0.8 + 0.2 * rng.random()))
    else:
        v[1:] = (rng.integers(1, 64, size=M - 1) / 64.0).astype(np.float32)
    return v


# ---------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------
def with_depot_visits(rng, customers, T, cls):
    """`customers` in order, filled to T steps with depot visits: `tail` of them at the end (0 for ends_at_customer, 1 for
    ends_at_depot, k >= 2 for pad_k), the others between two customers, never two in a row."""
    n, slack = len(customers), T - len(customers)
    if cls == "only_depot":
        return [0] * T
    if n == 1:                                               # a single customer: the depot before or after it
        return ([0] * slack + customers) if cls == "ends_at_customer" else (customers + [0] * slack)
    tail = {"ends_at_customer": 0, "ends_at_depot": 1}.get(cls)
    if tail is None:
        tail = int(rng.integers(2, slack + 1))
    inner = slack - tail
    assert 0 <= inner <= n - 1, (n, T, cls)
    cuts = set((rng.choice(n - 1, size=inner, replace=False) + 1).tolist())
    out = []
    for i, c in enumerate(customers):
        if i in cuts:
            out.append(0)
        out.append(int(c))
    return out + [0] * tail


def draw_row(rng, env, N, T, cls):
    if env == "tsp":
        return rng.permutation(N).tolist()
    if env == "pdp":
        perm = (rng.permutation(N) + 1).tolist()
        pos = {c: i for i, c in enumerate(perm)}
        for p in range(1, N // 2 + 1):                       # pickup p before its delivery p + N / 2
            d = p + N // 2
            if pos[d] < pos[p]:
                perm[pos[p]], perm[pos[d]] = d, p
                pos[p], pos[d] = pos[d], pos[p]
        return {"from_pickup": perm, "depot_start": [0] + perm, "ends_at_depot": perm + [0]}[cls]
    if cls == "only_depot":
        return [0] * T
    tail_min = {"ends_at_customer": 0, "ends_at_depot": 1, "pad_k": 2}[cls]
    if env == "cvrp":
        k = N
    else:                                                    # PCTSP / OP visit a subset
        top = min(N, T - tail_min)
        k = top if cls == "ends_at_customer" else int(rng.integers(max(1, top // 2), top + 1))
        k = max(k, (T - tail_min) // 2 + 1)                  # so that the depot visits in between fit
    return with_depot_visits(rng, (rng.permutation(N)[:k] + 1).tolist(), T, cls)


def rotate_tsp(locs, row, cls):
    """TSP: start the cycle so that its longest leg is the closing one (closing_long) or the first (first_long)."""
    if cls == "perm":
        return row
    p = locs[np.array(row)].astype(np.float64)
    j = int(np.argmax(np.sqrt(((np.roll(p, -1, axis=0) - p) ** 2).sum(-1))))       # leg j: row[j] -> row[j + 1]
    s = j + 1 if cls == "closing_long" else j
    return row[s:] + row[:s]


def edge_terms(env, g1):
    """The terms of a one-row group that the edges of the kernels' tiles single out: legs (between two different stops)
    and per-step values (at customers) at steps 0, 63, 64, 127, 128 and at the end."""
    a = g1["actions"][0]
    out = []
    if env != "op":
        d = rr.legs(g1["locs"], g1["actions"], g1["inst"], env != "tsp")[0]
        stops = a if env == "tsp" else np.concatenate([[0], a])
        P = d.size
        for t in set(EDGE_STEPS + (P - 2, P - 1)):
            if 0 <= t < P and stops[t] != stops[(t + 1) % P]:
                out.append(d[t])
    if env in ("pctsp", "op"):
        v = g1["penalty" if env == "pctsp" else "prize"][g1["inst"][0]]
        out += [float(v[a[t]]) for t in set(EDGE_STEPS + (a.size - 1,)) if 0 <= t < a.size and a[t] != 0]
    return out


def classes_for(env, N, T):
    if env == "tsp":
        return CLASSES["tsp"]
    if env == "pdp":
        return ("from_pickup",) if T == N else ("depot_start", "ends_at_depot")
    slack = T - N
    if env == "cvrp":
        return ("ends_at_customer",) + (("ends_at_depot",) if slack >= 1 else ()) + (("pad_k",) if slack >= 2 and N > 1 else ())
    return ("ends_at_customer", "ends_at_depot") + (("pad_k", "only_depot") if T >= 3 else ())


def build_group(rng, env, kind, N, T):
    M = N if env == "tsp" else N + 1
    g = {"kind": np.array(kind)}
    if "locs" in INSTANCE_KEYS[env]:
        g["locs"] = np.stack([make_locs(rng, kind, M) for _ in range(B)])
    if env == "pctsp":
        g["penalty"] = np.stack([make_node_values(rng, kind, M, 0.25) for _ in range(B)])
    if env == "op":
        g["prize"] = np.stack([make_node_values(rng, kind, M, 1.0) for _ in range(B)])
    inst = rng.permutation(np.arange(ROWS) % B)              # interleaved: no row order that r % B or r // S could mimic
    names = classes_for(env, N, T)
    rows, labels = [], []
    for r in range(ROWS):
        cls = names[r % len(names)]
        for attempt in range(50000):
            row = draw_row(rng, env, N, T, cls)
            if env == "tsp":
                row = rotate_tsp(g["locs"][inst[r]], row, cls)
            assert len(row) == T
            if kind != "generic" or cls == "only_depot":
                break
            g1 = dict(g, actions=np.array([row], np.int64), inst=inst[r:r + 1])
            floor = max(FLOOR, FLOOR_TOLS * float(rr.tol(evaluate(env, g1))[0]))
            if all(x >= floor for x in edge_terms(env, g1)):
                break
        else:
            raise AssertionError(f"{env} N {N} T {T} {cls}: no row clears the floor")
        rows.append(row)
        labels.append(cls)
    g["actions"] = np.array(rows, np.int64)
    g["inst"] = inst.astype(np.int64)
    g["cls"] = np.array(labels)
    return g


def build_logp_group(rng, kind, T):
    if kind == "generic":
        x = -(rng.random((ROWS, T), dtype=np.float32) * np.float32(4.0))
        for r in range(ROWS):                                # the terms at the tile edges stay away from zero
            floor = max(FLOOR, FLOOR_TOLS * float(rr.tol(rr.loglik(x[r:r + 1]))[0]))
            for t in set(EDGE_STEPS + (T - 1,)):
                while 0 <= t < T and -x[r, t] < floor:
                    x[r, t] = -(rng.random(dtype=np.float32) * np.float32(4.0))
    else:
        x = (-rng.integers(0, 8192, size=(ROWS, T)) / 1024.0).astype(np.float32)
        x[:, [0, T - 1]] = np.minimum(x[:, [0, T - 1]], np.float32(-1 / 1024))
    labels = np.array(["logp"] * ROWS, dtype="U9")
    if T >= 20:                                              # the log-prob 0 of padded steps: the last third of two rows
        x[ROWS - 2:, T - T // 3:] = 0.0
        labels[ROWS - 2:] = "zero_tail"
    return {"kind": np.array(kind), "logp": x, "cls": labels, "actions": np.zeros((ROWS, T), np.int64),
            "inst": np.arange(ROWS) % B}


def build(env, rng):
    groups = []
    shapes = {"tsp": [(n, n) for n in TSP_NODES], "pdp": PDP_SHAPES, "logp": [(0, t) for t in LOGP_STEPS]}.get(env, DEPOT_SHAPES)
    for N, T in shapes:
        for kind in KINDS:
            if env == "logp":
                if kind != "exact_y":                        # one exact kind: there are no coordinates
                    groups.append(build_logp_group(rng, "exact" if kind == "exact_x" else kind, T))
            else:
                groups.append(build_group(rng, env, kind, N, T))
    return groups


# ---------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------
class _Stub:
    check_solution = False                                   # all that a `_get_reward` reads from self (TSP's)


def _reference():
    import _refshim

    _refshim.install()
    import torch
    from tensordict import TensorDict  # the stand-in

    from rl4co.envs.routing.cvrp.env import CVRPEnv
    from rl4co.envs.routing.op.env import OPEnv
    from rl4co.envs.routing.pctsp.env import PCTSPEnv
    from rl4co.envs.routing.pdp.env import PDPEnv
    from rl4co.envs.routing.tsp.env import TSPEnv
    from rl4co.utils.decoding import get_log_likelihood

    torch.set_num_threads(1)
    stub = _Stub()
    fns = {"tsp": lambda td, a: TSPEnv._get_reward(stub, td, a), "cvrp": lambda td, a: CVRPEnv._get_reward(stub, td, a),
           "pdp": lambda td, a: PDPEnv._get_reward(td, a), "pctsp": lambda td, a: PCTSPEnv._get_reward(stub, td, a),
           "op": lambda td, a: OPEnv._get_reward(stub, td, a)}
    return torch, TensorDict, fns, get_log_likelihood


def reference_reward(env, g):
    torch, TensorDict, fns, get_log_likelihood = _reference()
    if env == "logp":
        out = get_log_likelihood(torch.from_numpy(g["logp"].copy()), return_sum=True)
    else:
        src = {k: torch.from_numpy(np.ascontiguousarray(g[k][g["inst"]])) for k in INSTANCE_KEYS[env]}
        td = TensorDict(src, batch_size=[g["actions"].shape[0]])
        out = fns[env](td, torch.from_numpy(g["actions"].copy()))
    assert out.dtype == torch.float32 and tuple(out.shape) == (g["actions"].shape[0],)
    return out.numpy().copy()


def reference_length_one(env, M):
    """The `T == 1` special case of PCTSP and OP: zeros for all-depot rows, an assertion otherwise."""
    torch, TensorDict, fns, _ = _reference()
    td = TensorDict({"locs": torch.rand(4, M, 2), "penalty": torch.rand(4, M), "prize": torch.rand(4, M)}, batch_size=[4])
    zero = fns[env](td, torch.zeros(4, 1, dtype=torch.int64)).numpy().copy()
    try:
        fns[env](td, torch.tensor([[0], [0], [1], [0]]))
        raise SystemExit(f"{env}: the reference accepts a length-1 tour to a customer")
    except AssertionError as e:
        return zero, str(e)


def main():
    for s, env in enumerate(ENVS):
        rng = np.random.default_rng(20251019 + s)
        groups = build(env, rng)
        out, rows, worst = {}, 0, 0.0
        for i, g in enumerate(groups):
            g["reward"] = reference_reward(env, g)
            res = evaluate(env, g)
            if str(g["kind"]) == "generic":
                worst = max(worst, used_fraction(g["reward"], res))
            else:                                            # bit for bit: float32(value) is exact and is what was recorded
                exact = res.value.astype(np.float32)
                assert (exact.astype(np.float64) == res.value).all(), f"{env} group {i}: not representable"
                assert (g["reward"] == exact).all(), f"{env} group {i}: reference != float64 on an exact group"
            rows += g["reward"].size
            for k, v in g.items():
                out[f"g{i}_{k}"] = v.astype(np.int16) if k in ("actions", "inst") else v
        out["groups"] = np.int64(len(groups))
        if env in ("pctsp", "op"):
            zero, msg = reference_length_one(env, 5)
            assert msg.startswith(T1_MESSAGE), msg
            out["t1_zero_reward"], out["t1_message"] = zero, np.array(msg)
        labels = np.concatenate([g["cls"] for g in groups])
        missing = [c for c in CLASSES[env] if c not in labels]
        assert not missing, f"{env}: no row of class {missing}"
        Ts = {g["actions"].shape[1] for g in groups}
        Ps = {leg_count(env, g) for g in groups}
        assert set(EDGE) <= Ts and set(EDGE) <= Ps, (env, sorted(Ts), sorted(Ps))
        path = os.path.join(HERE, f"reward_{env}.npz")
        write_npz(path, out)
        size = os.path.getsize(path)
        assert size < 256 * 1024, (env, size)
        shapes = sorted({tuple(g["actions"].shape) for g in groups})
        print(f"reward_{env}: rows {rows} groups {len(groups)} shapes {shapes} {size} bytes, "
              f"worst used fraction of tol (reference vs float64, generic rows) {worst:.3f}", flush=True)


if __name__ == "__main__":
    main()
