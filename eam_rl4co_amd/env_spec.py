"""What the host code knows about each routing env's flat rollout state (struct eamrl_state), stated once: one frozen
record per kernel family, read by `policy`, `ops`, `train` and `envs` instead of branching on the env name.  Data only, and
no import of the package's other modules, so all of them can import this one."""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

f32, i64, u8, bool_ = torch.float32, torch.int64, torch.uint8, torch.bool

# arguments of `step`, `reward` and `check`: a pseudo-argument -- the action(s) ([R] for a step, the [R, T] tours otherwise),
# M - 1, the capacities ([R], or the td's [B, 1]) --, "=text" for the literal text (the env name the check kernel takes), any
# other string for a TensorDict key; None and bools pass through
ACTION, NUM_LOC, VCAP = "<action>", "<num_loc>", "<vcap>"


class Field(NamedTuple):
    """One eamrl_state slot of an env.  Shapes: what follows the batch dimension, in terms of "M" (nodes) and "M-1"."""
    slot: str                               # member of struct eamrl_state
    key: str                                # TensorDict key it is read from (and written back to, if `emit`)
    dtype: torch.dtype                      # on the device
    shape: Tuple                            # in the TensorDict, after `transform`; a per-row (1,) is flat [R] on the device
    meaning: str
    per_row: bool = True                    # [R, ...], replicated for multistart; else per instance [B, ...], shared
    reset: str = "zeros"                    # RolloutState.__init__: zeros | ones | depot | depot_and_pickups (per row only)
    emit: bool = True                       # state_to_td writes it back under `key` (per row only)
    transform: Optional[str] = None         # "col0": take [..., 0];  "not": logical negation (and back when emitted)
    src_dtype: Optional[torch.dtype] = None  # in the TensorDict, where it differs from `dtype` (emitted as that again)


class EnvSpec(NamedTuple):
    name: str
    abi_id: int                             # EAMRL_ENV_* of include/eamrl.h
    max_steps: Tuple[int, int, bool]        # (a, b, minus_npre): a * M + b (- the multistart pre-steps)
    has_pb: bool                            # the cache has a Pb plane (projection of the first node)
    n_state_cols: int                       # state columns of project_context (rows of cvec, planes of `sc`)
    fields: Tuple[Field, ...]               # in the key order of state_to_td
    step: Tuple[str, Tuple]                 # ops step wrapper, its positional arguments as slots / ACTION / None
    reward: Tuple[str, Tuple]               # ops reward function, its positional arguments
    check: Tuple[str, Tuple]                # ops check function -> int32[2] counters of bad rows, its arguments
    messages: Tuple[str, str]               # the assertion messages of counters 0 and 1
    check_padded: str                       # on depot-padded tours?  yes | no | if_full (TSP: only unpadded, node 0 is a city)
    reeval_static: Tuple[str, ...]          # TensorDict keys the re-evaluation's state replay reads


_CUR, _CUR1 = (Field("cur", "current_node", i64, s, "node the vehicle is at") for s in ((), (1,)))
_VISITED_U8 = Field("visited", "visited", u8, ("M",), "1 = node visited")
_VISITED_BOOL = Field("visited", "visited", bool_, ("M",), "node visited")
_ISTEP = Field("istep", "i", i64, (), "steps taken")
_LOCS = Field("locs", "locs", f32, ("M", 2), "node coordinates", per_row=False)
_TOUR_WITH_DEPOT = ("tour_length_reward", ("locs", ACTION, True))
_CVRP_CHECK = ("check_solution", ("=cvrp", ACTION, "demand", VCAP))
_CVRP_MESSAGES = ("Invalid tour", "Used more than capacity")
_CVRP_HEAD = (_CUR1, Field("used", "used_capacity", f32, (1,), "load picked up since the last depot visit"),
              Field("vcap", "vehicle_capacity", f32, (1,), "vehicle capacity", reset="ones"))
_DEMAND = Field("demand", "demand", f32, ("M-1",), "demand per customer", per_row=False)

ENV_SPECS = {s.name: s for s in (
    EnvSpec("tsp", 0, (1, 0, True), has_pb=True, n_state_cols=0,        # one step per remaining node
            fields=(Field("first", "first_node", i64, (), "first node of the tour"), _CUR, _ISTEP._replace(shape=(1,))),
            step=("tsp_step_", ("mask", "first", "cur", "istep", ACTION, "done")),
            reward=("tour_length_reward", ("locs", ACTION, False)),
            check=("check_solution", ("=tsp", ACTION)), messages=_CVRP_MESSAGES, check_padded="if_full", reeval_static=()),
    EnvSpec("cvrp", 1, (2, 1, False), has_pb=False, n_state_cols=1,     # a customer visit, then at most one depot visit
            fields=_CVRP_HEAD + (_VISITED_U8, _DEMAND),
            step=("cvrp_step_mask_", ("visited", "used", "vcap", "demand", "cur", ACTION, "mask", "done")),
            reward=_TOUR_WITH_DEPOT, check=_CVRP_CHECK, messages=_CVRP_MESSAGES, check_padded="yes",
            reeval_static=("demand", "vehicle_capacity")),
    # SDVRP: the reference's validity replay starts from (-capacity, demand...) and its verdict depends on where the action
    # tensor ends, so it runs on the exact [R, T] slice rather than on the padded one
    EnvSpec("sdvrp", 2, (3, 1, False), has_pb=False, n_state_cols=1,    # as CVRP plus at most one split delivery per trip
            fields=_CVRP_HEAD + (Field("rem", "demand_with_depot", f32, ("M",), "demand left per node (depot slot 0)"), _DEMAND),
            step=("sdvrp_step_mask_", ("rem", "used", "vcap", "cur", ACTION, "mask", "done")),
            reward=_TOUR_WITH_DEPOT, check=("check_solution", ("=sdvrp", ACTION, "demand", VCAP)), check_padded="no",
            messages=("All demand must be satisfied", "Cannot visit depot twice if any nonzero demand"),
            reeval_static=("demand", "vehicle_capacity")),
    # PCTSP: cur_total_penalty is bookkeeping of env.step only (no decision reads it): the fused rollout does not carry it
    EnvSpec("pctsp", 3, (1, 1, False), has_pb=False, n_state_cols=1,
            fields=(_CUR, Field("used", "cur_total_prize", f32, (), "pctsp: prize collected so far"),
                    Field("vcap", "prize_required", f32, (), "pctsp: prize required", reset="ones"), _VISITED_BOOL, _ISTEP,
                    Field("demand", "real_prize", f32, ("M",), "pctsp: prize per node (depot slot 0)", per_row=False)),
            step=("pctsp_step_mask_", ("visited", "used", None, "demand", None, "cur", "istep", ACTION, "mask", "done")),
            reward=("pctsp_reward", ("locs", "penalty", ACTION)),   # depot padding: zero-length legs, zero penalties: exact
            check=("check_solution", ("=pctsp", ACTION, "real_prize")), check_padded="yes",
            messages=("Duplicates", "Total prize does not satisfy min total prize"),
            reeval_static=("real_prize", "prize_required")),
    # OP: current_total_prize is bookkeeping of env.step only (the reward is recomputed from the actions)
    EnvSpec("op", 4, (1, 1, False), has_pb=False, n_state_cols=1,
            fields=(_CUR1, Field("used", "tour_length", f32, (), "op: tour length so far"),
                    Field("vcap", "max_length", f32, (), "op: the instance's max_length[:, 0]", reset="ones", emit=False,
                          transform="col0"), _VISITED_BOOL, _ISTEP,
                    Field("demand", "max_length", f32, ("M",), "op: arrival limit per node", per_row=False), _LOCS),
            step=("op_step_mask_", ("visited", "used", None, None, "locs", "demand", "cur", "istep", ACTION, "mask", "done")),
            reward=("op_reward", ("prize", ACTION)),                # depot padding adds zero prizes
            check=("op_check_solution", (ACTION, "locs", "max_length")), check_padded="yes",
            messages=("Duplicates", "Max length exceeded"), reeval_static=("locs", "max_length")),
    EnvSpec("cvrptw", 5, (2, 1, False), has_pb=False, n_state_cols=2,   # state columns: capacity | time
            fields=_CVRP_HEAD + (
                _VISITED_U8, Field("time", "current_time", f32, (1,), "the vehicle's clock"), _DEMAND, _LOCS, Field("tw", "time_windows", f32, ("M", 2), "service window per node", False, src_dtype=torch.int32),
                Field("dur", "durations", f32, ("M",), "service time per node", per_row=False)),
            step=("cvrptw_step_mask_", ("visited", "used", "vcap", "demand", "cur", "time", "locs", "tw", "dur", ACTION,
                                        "mask", "done")),
            reward=_TOUR_WITH_DEPOT, check=_CVRP_CHECK, messages=_CVRP_MESSAGES,    # (CVRP's) + the env class's time replay,
            check_padded="no",                                                      # which needs the exact slice
            reeval_static=("demand", "vehicle_capacity", "locs", "time_windows", "durations")),
    # PDP: N steps, N + 1 with force_start_at_depot (`_enqueue` takes the exact count); no state column (PDPContext is the
    # current node alone, eamrl_cache.cvec = NULL); "i" has no slot: `_finish`, which knows the number of steps, advances it
    EnvSpec("pdp", 6, (1, 0, True), has_pb=False, n_state_cols=0,
            fields=(_CUR1, Field("visited", "available", u8, ("M",), "pdp: 1 = no longer available (~available)",
                                 reset="depot", transform="not", src_dtype=bool_),
                    Field("to_deliver", "to_deliver", u8, ("M",), "pdp: 1 = depot, pickup, or delivery whose pickup is done",
                          reset="depot_and_pickups", src_dtype=bool_)),
            step=("pdp_step_mask_", ("visited", "to_deliver", "cur", ACTION, "mask", "done")),
            reward=_TOUR_WITH_DEPOT, check=("check_solution", ("=pdp", ACTION, None, None, NUM_LOC)), check_padded="yes",
            messages=("Not visiting all nodes", "Deliverying without pick-up"),
            reeval_static=("available", "to_deliver", "action_mask")),
)}

# envs that share kernels, embeddings and state layout with another one: SPCTSP is PCTSP whose collected prize is the
# stochastic one (the policy sees the expected prize either way)
ALIASES = {"spctsp": "pctsp"}


def spec(env_name: str) -> EnvSpec:
    return ENV_SPECS[ALIASES.get(env_name, env_name)]


def dims(shape, M: int, device: bool = False):
    """`shape` with "M" / "M-1" filled in; device=True: as the kernels see it (a per-row scalar is [R], never [R, 1])."""
    shape = shape[:-1] if device and shape[-1:] == (1,) else shape
    return tuple(M if d == "M" else M - 1 if d == "M-1" else d for d in shape)


def max_steps(env_name: str, M: int, npre: int = 0) -> int:
    """Upper bound of the decode steps of one rollout after `npre` multistart pre-steps."""
    a, b, minus_npre = ENV_SPECS[env_name].max_steps
    return a * M + b - (npre if minus_npre else 0)
