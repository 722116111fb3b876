"""What test_host_reward.py and test_gpu_reward.py share: the committed reward fixtures with the float64 restatement's
Result next to each group (computed once, read-only), which mutants of the restatement a group must catch, the oracle's
value of a group's rows, and the multistart case built on top of the fixtures."""
import os

import numpy as np

import make_golden_reward as mk
import reward_ref as rr
from _util import GOLDEN

ENVS = mk.ENVS
TOUR_ENVS = ("tsp", "cvrp", "pdp")
_cache, _extra = {}, {}


def fixture(env):
    """The groups of reward_<env>.npz with the restatement's Result (`ref`) and its tolerance (`tol`) next to each."""
    if env not in _cache:
        path = os.path.join(GOLDEN, f"reward_{env}.npz")
        groups = mk.load_groups(path)
        for g in groups:
            g["kind"] = str(g["kind"].reshape(-1)[0])
            g["ref"] = mk.evaluate(env, g)
            g["tol"] = rr.tol(g["ref"])
            for v in (*g.values(), *g["ref"]):
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        with np.load(path) as z:
            _extra[env] = {k: z[k] for k in z.files if k.startswith("t1_")}
        _cache[env] = groups
    return _cache[env]


def length_one(env):
    """The reference's recorded `T == 1` behaviour of PCTSP / OP: (reward of all-depot rows, assertion message)."""
    fixture(env)
    return _extra[env]["t1_zero_reward"], str(_extra[env]["t1_message"].reshape(-1)[0])


def exact(g):
    return g["kind"] != "generic"


def mutants_for(env, g):
    """The mutants of reward_ref that change what this group's rows are worth."""
    T, P = g["actions"].shape[1], mk.leg_count(env, g)
    out = ["sign"]
    if env in ("op", "logp"):
        return out + ["saved_short"] + (["first64"] if T > 64 else [])
    out += ["no_closing"] + (["no_first"] if env != "tsp" else []) + (["no_leg63"] if P >= 64 else [])
    out += (["first64"] if P > 64 else []) + (["no_y"] if g["kind"] != "exact_x" else [])
    return out + (["pen_shifted", "saved_short"] if env == "pctsp" else [])


def oracle_value(orc, env, g, actions=None, inst=None, rows=None):
    """The CPU oracle on rows of a group, row r against its own instance (B = R)."""
    rows = np.arange(g["actions"].shape[0]) if rows is None else rows
    if env == "logp":
        return orc.sum_logp(g["logp"][rows] if actions is None else actions)
    a = g["actions"][rows] if actions is None else actions
    i = g["inst"][rows] if inst is None else inst
    if env == "pctsp":
        return orc.pctsp_reward(g["locs"][i], g["penalty"][i], a)
    if env == "op":
        return orc.op_reward(g["prize"][i], a)
    return orc.tour_length_reward(g["locs"][i], a, env != "tsp")


def multistart_case(env, S, group):
    """S * B rows in "(s b)" order over the B = 3 instances of one fixture group: row r is a tour of instance r % B.
    -> (the group, actions [S * B, T], Result with the r % B reading, Result with the wrong r // S reading)."""
    g = fixture(env)[group]
    rows = []
    for s in range(S):
        for b in range(mk.B):
            mine = np.flatnonzero(g["inst"] == b)
            rows.append(g["actions"][mine[s % mine.size]])
    actions = np.stack(rows)
    R = S * mk.B
    return g, actions, mk.evaluate(env, g, actions, np.arange(R) % mk.B), mk.evaluate(env, g, actions, np.arange(R) // S)


def multistart_groups(env):
    """One exact and one generic group with more than 64 legs, by index."""
    groups = fixture(env)
    return [next(i for i, g in enumerate(groups) if g["kind"] == k and g["actions"].shape[1] == 70 - 5 * (env in ("tsp", "pdp")))
            for k in ("exact_x", "generic")]
