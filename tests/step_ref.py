"""The step-and-mask rule of every routing env as a plain numpy state machine, one row at a time.

Written from the reference env sources (`_reset`, `_step`, `get_action_mask` of rl4co/envs/routing/*/env.py), not from the
kernels and not from oracle/.  tests/test_host_step_ref.py pins it, bit for bit, to states recorded from the unmodified
reference (step_boundary.npz, env_*_random.npz); tests/test_gpu_step_rule.py then holds the five device restatements of
the rule to it.

The rule is a float32 rule: the reference env runs float32 torch on the CPU, so every arithmetic step here is one
np.float32 operation in the reference's operation order (`vcap + 1e-5` is one float32 add).  A float64 reference would be
wrong by construction: where a load, an arrival or a prize total sits on a comparison boundary, float64 arithmetic gives
a different verdict from the reference's, and those rows are exactly what this module exists for.

The one composite operation is the Euclidean leg.  torch's CPU `norm(p=2, dim=-1)` of a 2-vector (dx, dy) is
sqrt(fma(dy, dy, dx * dx)): the product dx * dx rounded to float32, dy * dy added to it unrounded, one rounding, then a
correctly rounded square root.  The three other candidates (`LEG_FORMULAS`) differ from the recorded tour lengths and
clocks; test_host_step_ref.py::test_leg_formula_is_the_one_the_reference_uses shows it.

    instance  dict of ONE instance's arrays in the generators' vocabulary, plus "env":
                tsp     locs [M, 2]
                cvrp    depot [2], locs [N, 2], demand [N]                     (sdvrp alike)
                cvrptw  cvrp's + time_windows [M, 2] int32, durations [M]
                pctsp   depot, locs, deterministic_prize [N], stochastic_prize [N], penalty [N]      (spctsp alike)
                op      depot, locs, prize [N], max_length ()
                pdp     depot, locs [N, 2]
    state     dict: the slots env_spec.ENV_SPECS[env].fields lists (under their slot names) + "mask", "done", "env", and the
              bookkeeping the reference's step keeps besides ("pen_tot", "prize_tot")

reset(instance) -> state;  step(state, action) -> a new state (the old one is left as it was).
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

f32 = np.float32
ZERO, ONE = f32(0.0), f32(1.0)


# ---------------------------------------------------------------------------------------------------------------------
# float32 pieces
# ---------------------------------------------------------------------------------------------------------------------
def round_to_f32(x: Fraction) -> np.float32:
    """The float32 nearest to the non-negative rational x, ties to even (no overflow handling: legs are small)."""
    if x == 0:
        return ZERO
    assert x > 0
    n, d = x.numerator, x.denominator
    e = n.bit_length() - d.bit_length() - 24          # 2^23 <= x / 2^e < 2^25, narrowed below
    while Fraction(n, d) / Fraction(2) ** e >= 1 << 24:
        e += 1
    while Fraction(n, d) / Fraction(2) ** e < 1 << 23:
        e -= 1
    e = max(e, -149)                                   # subnormals keep the smallest exponent
    q = Fraction(n, d) / Fraction(2) ** e
    m = q.numerator // q.denominator
    rest = q - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and (m & 1)):
        m += 1
    return f32(float(Fraction(m) * Fraction(2) ** e))  # m < 2^25 and a power of two: exact in float64, exact in float32


def fma32(a, b, c) -> np.float32:
    """a * b + c with one rounding."""
    return round_to_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _leg_fma_y(dx, dy):
    return np.sqrt(fma32(dy, dy, f32(dx * dx)))


def _leg_fma_x(dx, dy):
    return np.sqrt(fma32(dx, dx, f32(dy * dy)))


def _leg_plain(dx, dy):
    return np.sqrt(f32(f32(dx * dx) + f32(dy * dy)))


def _leg_f64(dx, dy):
    return f32(np.sqrt(np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy)))


LEG_FORMULAS = {"fma_y": _leg_fma_y, "fma_x": _leg_fma_x, "plain": _leg_plain, "float64": _leg_f64}
LEG = "fma_y"       # the one that reproduces the reference's recorded tour lengths and clocks


@functools.lru_cache(maxsize=None)
def _leg_of(formula, dx, dy):
    return LEG_FORMULAS[formula](f32(dx), f32(dy))


def leg(p, q, formula=None) -> np.float32:
    """(p - q).norm(p=2, dim=-1) of two float32 points (remembered per difference: the exact fma is slow)."""
    dx, dy = f32(p[0] - q[0]), f32(p[1] - q[1])
    return _leg_of(formula or LEG, float(dx), float(dy))


def _with_depot(inst):
    return np.concatenate([np.asarray(inst["depot"], f32)[None], np.asarray(inst["locs"], f32)], 0)


# ---------------------------------------------------------------------------------------------------------------------
# TSP (tsp/env.py:62-115)
# ---------------------------------------------------------------------------------------------------------------------
def _tsp_reset(inst):
    M = np.asarray(inst["locs"]).shape[0]
    return {"env": "tsp", "first": 0, "cur": 0, "istep": 0, "mask": np.ones(M, bool), "done": False}


def _tsp_step(s, a):
    n = dict(s)
    # (the reference takes `first_node` for the whole batch while any row has i == 0; its rows all share one i)
    n["first"] = a if s["istep"] == 0 else s["first"]
    n["mask"] = s["mask"].copy()
    n["mask"][a] = False
    n["done"] = not n["mask"].any()
    n["cur"], n["istep"] = a, s["istep"] + 1
    return n


# ---------------------------------------------------------------------------------------------------------------------
# CVRP (cvrp/env.py:68-144) and CVRPTW (cvrptw/env.py:99-161)
# ---------------------------------------------------------------------------------------------------------------------
def _cvrp_mask(s):
    N = s["demand"].shape[0]
    lim = f32(s["vcap"] + f32(1e-5))
    mask_loc = np.zeros(N, bool)
    for j in range(N):
        exceeds = f32(s["demand"][j] + s["used"]) > lim
        mask_loc[j] = bool(s["visited"][j + 1]) or exceeds
    free = 0
    for j in range(N):
        free += int(not mask_loc[j])
    mask = np.empty(N + 1, bool)
    mask[0] = not (s["cur"] == 0 and free > 0)
    mask[1:] = ~mask_loc
    return mask


def _cvrptw_mask(s):
    mask = _cvrp_mask(s)
    M = mask.shape[0]
    for n in range(M):
        arrive = f32(s["time"] + leg(s["locs"][s["cur"]], s["locs"][n]))
        mask[n] = mask[n] and bool(arrive <= s["tw"][n, 1])
    return mask


def _cvrp_reset(inst, tw=False):
    N = np.asarray(inst["demand"]).shape[0]
    s = {"env": "cvrptw" if tw else "cvrp", "cur": 0, "used": ZERO, "vcap": f32(inst.get("vehicle_capacity", 1.0)),
         "visited": np.zeros(N + 1, np.uint8), "demand": np.asarray(inst["demand"], f32), "done": False}
    if tw:
        s["time"] = ZERO
        s["locs"] = _with_depot(inst)
        s["tw"] = np.asarray(inst["time_windows"]).astype(f32)      # int32 in the reference; it compares in float32
        s["dur"] = np.asarray(inst["durations"], f32)
    s["mask"] = _cvrptw_mask(s) if tw else _cvrp_mask(s)
    return s


def _cvrp_step(s, a):
    n = dict(s)
    N = s["demand"].shape[0]
    tw = s["env"] == "cvrptw"
    if tw:      # the clock moves first, from the node the vehicle is still at
        arrive = f32(s["time"] + leg(s["locs"][s["cur"]], s["locs"][a]))
        start = arrive if arrive >= s["tw"][a, 0] else s["tw"][a, 0]
        n["time"] = f32(f32(a != 0) * f32(start + s["dur"][a]))
    selected = s["demand"][min(max(a - 1, 0), N - 1)]       # (the clamp makes the depot read the first customer's demand)
    n["used"] = f32(f32(s["used"] + selected) * f32(a != 0))
    n["visited"] = s["visited"].copy()
    n["visited"][a] = 1
    n["done"] = int(n["visited"].sum()) == N + 1
    n["cur"] = a
    n["mask"] = _cvrptw_mask(n) if tw else _cvrp_mask(n)
    return n


# ---------------------------------------------------------------------------------------------------------------------
# SDVRP (sdvrp/env.py:58-135)
# ---------------------------------------------------------------------------------------------------------------------
def _sdvrp_mask(s):
    M = s["rem"].shape[0]
    full = s["used"] >= s["vcap"]
    mask = np.empty(M, bool)
    free = 0
    for n in range(1, M):
        blocked = bool(s["rem"][n] == 0) or bool(full)
        mask[n] = not blocked
        free += int(not blocked)
    mask[0] = not (s["cur"] == 0 and free > 0)
    return mask


def _sdvrp_reset(inst):
    demand = np.asarray(inst["demand"], f32)
    s = {"env": "sdvrp", "cur": 0, "used": ZERO, "vcap": f32(inst.get("vehicle_capacity", 1.0)),
         "rem": np.concatenate([np.zeros(1, f32), demand]), "demand": demand, "done": False}
    s["mask"] = _sdvrp_mask(s)
    return s


def _sdvrp_step(s, a):
    n = dict(s)
    selected = s["rem"][a]
    free_cap = f32(s["vcap"] - s["used"])
    delivered = selected if selected <= free_cap else free_cap
    n["used"] = f32(f32(s["used"] + delivered) * f32(a != 0))
    n["rem"] = s["rem"].copy()
    n["rem"][a] = f32(s["rem"][a] + f32(-delivered))
    n["done"] = not any(bool(v > 0) for v in n["rem"])
    n["cur"] = a
    n["mask"] = _sdvrp_mask(n)
    return n


# ---------------------------------------------------------------------------------------------------------------------
# PCTSP / SPCTSP (pctsp/env.py:64-156)
# ---------------------------------------------------------------------------------------------------------------------
def _pctsp_mask(s):
    M = s["visited"].shape[0]
    mask = np.empty(M, bool)
    seen = 0
    for n in range(1, M):
        mask[n] = not (s["visited"][n] or s["visited"][0])
        seen += int(s["visited"][n])
    mask[0] = not (bool(s["used"] < ONE) and seen < M - 1)
    return mask


def _pctsp_reset(inst, stochastic=False):
    real = np.asarray(inst["stochastic_prize" if stochastic else "deterministic_prize"], f32)
    penalty = np.asarray(inst["penalty"], f32)
    pen_tot = ZERO
    for p in penalty:       # (bookkeeping only: no decision reads it; torch sums pairwise, so it is compared loosely)
        pen_tot = f32(pen_tot + p)
    s = {"env": "spctsp" if stochastic else "pctsp", "cur": 0, "used": ZERO, "vcap": ONE,
         "visited": np.zeros(real.shape[0] + 1, bool), "istep": 0, "demand": np.concatenate([np.zeros(1, f32), real]),
         "penalty": np.concatenate([np.zeros(1, f32), penalty]), "pen_tot": pen_tot, "done": False}
    s["mask"] = _pctsp_mask(s)
    return s


def _pctsp_step(s, a):
    n = dict(s)
    n["used"] = f32(s["used"] + s["demand"][a])
    n["pen_tot"] = f32(s["pen_tot"] + s["penalty"][a])
    n["visited"] = s["visited"].copy()
    n["visited"][a] = True
    n["done"] = s["istep"] > 0 and a == 0
    n["cur"], n["istep"] = a, s["istep"] + 1
    n["mask"] = _pctsp_mask(n)
    return n


# ---------------------------------------------------------------------------------------------------------------------
# OP (op/env.py:69-164)
# ---------------------------------------------------------------------------------------------------------------------
def _op_mask(s):
    M = s["visited"].shape[0]
    mask = np.empty(M, bool)
    for n in range(M):
        exceeds = f32(s["used"] + leg(s["locs"][n], s["locs"][s["cur"]])) > s["demand"][n]
        mask[n] = not (s["visited"][n] or s["visited"][0] or bool(exceeds))
    mask[0] = True
    return mask


def _op_reset(inst):
    locs = _with_depot(inst)
    M = locs.shape[0]
    limit = np.empty(M, f32)
    for n in range(M):      # the arrival limit per node: what is left after the way back, minus a margin
        limit[n] = f32(f32(f32(inst["max_length"]) - leg(locs[0], locs[n])) - f32(1e-6))
    s = {"env": "op", "cur": 0, "used": ZERO, "vcap": limit[0], "visited": np.zeros(M, bool), "istep": 0, "demand": limit,
         "locs": locs, "prize": np.concatenate([np.zeros(1, f32), np.asarray(inst["prize"], f32)]), "prize_tot": ZERO,
         "done": False}
    s["mask"] = _op_mask(s)
    return s


def _op_step(s, a):
    n = dict(s)
    n["used"] = f32(s["used"] + leg(s["locs"][a], s["locs"][s["cur"]]))
    n["prize_tot"] = f32(s["prize_tot"] + s["prize"][a])
    n["visited"] = s["visited"].copy()
    n["visited"][a] = True
    n["done"] = a == 0 and s["istep"] > 0
    n["cur"], n["istep"] = a, s["istep"] + 1
    n["mask"] = _op_mask(n)
    return n


# ---------------------------------------------------------------------------------------------------------------------
# PDP: pdp_ref's state machine (pdp/env.py:66-240), one row of it
# ---------------------------------------------------------------------------------------------------------------------
def _pdp_state(env):
    return {"env": "pdp", "_env": env, "cur": int(env.current_node[0]), "visited": (~env.available[0]).astype(np.uint8),
            "to_deliver": env.to_deliver[0].astype(np.uint8), "mask": env.action_mask[0].copy(), "done": bool(env.done[0])}


def _pdp_reset(inst):
    import pdp_ref

    return _pdp_state(pdp_ref.Env(1, np.asarray(inst["locs"]).shape[0]))


def _pdp_step(s, a):
    import copy

    env = copy.deepcopy(s["_env"])
    env.step(np.array([a], np.int64))
    return _pdp_state(env)


RULES = {"tsp": (_tsp_reset, _tsp_step), "cvrp": (_cvrp_reset, _cvrp_step),
         "cvrptw": (lambda inst: _cvrp_reset(inst, tw=True), _cvrp_step), "sdvrp": (_sdvrp_reset, _sdvrp_step),
         "pctsp": (_pctsp_reset, _pctsp_step), "spctsp": (lambda inst: _pctsp_reset(inst, stochastic=True), _pctsp_step),
         "op": (_op_reset, _op_step), "pdp": (_pdp_reset, _pdp_step)}


def reset(instance):
    return RULES[str(instance["env"])][0](instance)


def step(state, action):
    a = int(action)
    assert 0 <= a < state["mask"].shape[0]
    return RULES[state["env"]][1](state, a)


# ---------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------
PER_INSTANCE = ("locs", "depot", "demand", "time_windows", "durations", "deterministic_prize", "stochastic_prize", "penalty",
                "prize", "max_length")


def instance(batch, b):
    """Instance b of a batch dict (arrays with a leading B, plus "env")."""
    out = {"env": str(batch["env"])}
    for k in PER_INSTANCE:
        if k in batch:
            out[k] = np.asarray(batch[k])[b]
    return out


def num_instances(batch):
    return np.asarray(batch["locs"]).shape[0]


def reset_rows(batch, S=1):
    """The R = S * B reset states in the device's row order: row r belongs to instance r % B."""
    B = num_instances(batch)
    return [reset(instance(batch, r % B)) for r in range(S * B)]


def first_feasible(mask, pref):
    for n in pref:
        if mask[n]:
            return int(n)
    raise AssertionError("no feasible action")


def rollout_first_feasible(batch, prefs, start_state=None):
    """Every row takes the first node of prefs[r, t] its mask allows; all rows keep stepping until every row is done, as
    the reference's decode loop does.  prefs [R, T, M]: a permutation of the nodes per row and step.
    -> (actions [R, T'], feasible [R, T'] = the number of feasible actions before each step, the list of final states,
        masks [R, T' + 1, M] = the mask before every step and after the last)."""
    prefs = np.asarray(prefs)
    R = prefs.shape[0]
    B = num_instances(batch)
    assert R % B == 0
    states = list(start_state) if start_state is not None else reset_rows(batch, R // B)
    actions, counts, masks = [], [], [np.stack([s["mask"] for s in states])]
    t = 0
    while not all(s["done"] for s in states):
        assert t < prefs.shape[1], "the preferences ran out before every row was done"
        acts = [first_feasible(s["mask"], prefs[r, t]) for r, s in enumerate(states)]
        counts.append([int(s["mask"].sum()) for s in states])
        states = [step(s, a) for s, a in zip(states, acts)]
        actions.append(acts)
        masks.append(np.stack([s["mask"] for s in states]))
        t += 1
    return (np.array(actions, np.int64).reshape(t, R).T.copy(), np.array(counts, np.int64).reshape(t, R).T.copy(), states,
            np.stack(masks, 1))


def replay(batch, actions, S=1, start_state=None):
    """The states after reset and after every column of actions [R, T] -> list of T + 1 lists of R states."""
    actions = np.asarray(actions)
    states = list(start_state) if start_state is not None else reset_rows(batch, S)
    out = [states]
    for t in range(actions.shape[1]):
        states = [step(s, a) for s, a in zip(states, actions[:, t])]
        out.append(states)
    return out
