"""The TensorDict <-> flat rollout state mapping of every env, stated a second time: what `state_from_td`, `state_to_td`,
`ops.RolloutState`, `ops._validate_state` and `_env_step_` have to give is written out here per env as expressions of the
TensorDict, independently of the table in eam_rl4co_amd/env_spec.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, N = 3, 6
f32, i64, u8, bl = torch.float32, torch.int64, torch.uint8, torch.bool

CASES = [("tsp", {}), ("cvrp", {}), ("sdvrp", {}), ("cvrptw", {}), ("pctsp", {}), ("spctsp", {}), ("op", {}), ("pdp", {}),
         ("pdp", {"force_start_at_depot": True})]
IDS = [n + ("-depot" if kw else "") for n, kw in CASES]
KIND = {"spctsp": "pctsp"}
SLOTS = ("first", "cur", "istep", "used", "vcap", "demand", "visited", "rem", "locs", "time", "tw", "dur", "to_deliver")


def make(name, kw):
    import eam_rl4co_amd as ea

    torch.manual_seed(1234)
    env = ea.get_env(name, generator_params=dict(num_loc=N), **kw)
    return env, env.reset(batch_size=[B]).to(DEV)


def expected(kind, td):
    """slot -> (per row?, dtype on the device, values [B, ...], the td key whose storage a copy=False state shares | None)."""
    row = lambda k: td[k].reshape(B)                       # scalars are [B] or [B, 1] in the TensorDict, [R] on the device
    if kind == "tsp":
        return {"first": (True, i64, row("first_node"), "first_node"), "cur": (True, i64, row("current_node"), "current_node"),
                "istep": (True, i64, row("i"), "i")}
    if kind == "pdp":       # the kernels keep the complement of `available`; both planes as bytes
        return {"cur": (True, i64, row("current_node"), "current_node"),
                "visited": (True, u8, (~td["available"]).to(u8), None),
                "to_deliver": (True, u8, td["to_deliver"].to(u8), None)}
    if kind == "op":        # used: tour length so far; vcap: the depot's entry of max_length; demand: the arrival limits
        return {"cur": (True, i64, row("current_node"), "current_node"), "istep": (True, i64, row("i"), "i"),
                "used": (True, f32, row("tour_length"), "tour_length"), "vcap": (True, f32, td["max_length"][:, 0], None),
                "visited": (True, bl, td["visited"], "visited"), "demand": (False, f32, td["max_length"], "max_length"),
                "locs": (False, f32, td["locs"], "locs")}
    if kind == "pctsp":     # used: prize collected so far; vcap: prize required; demand: prize per node
        return {"cur": (True, i64, row("current_node"), "current_node"), "istep": (True, i64, row("i"), "i"),
                "used": (True, f32, row("cur_total_prize"), "cur_total_prize"),
                "vcap": (True, f32, row("prize_required"), "prize_required"),
                "visited": (True, bl, td["visited"], "visited"), "demand": (False, f32, td["real_prize"], "real_prize")}
    out = {"cur": (True, i64, row("current_node"), "current_node"), "used": (True, f32, row("used_capacity"), "used_capacity"),
           "vcap": (True, f32, row("vehicle_capacity"), "vehicle_capacity"), "demand": (False, f32, td["demand"], "demand")}
    if kind == "sdvrp":
        out["rem"] = (True, f32, td["demand_with_depot"], "demand_with_depot")
    else:
        out["visited"] = (True, u8, td["visited"], "visited")
    if kind == "cvrptw":
        out.update({"time": (True, f32, row("current_time"), "current_time"), "locs": (False, f32, td["locs"], "locs"),
                    "tw": (False, f32, td["time_windows"].to(f32), None), "dur": (False, f32, td["durations"], "durations")})
    return out


# what state_to_td emits from the state, besides action_mask / done / reward: key -> (dtype, shape after R; "M" = nodes)
EMITTED = {
    "tsp": {"first_node": (i64, ()), "current_node": (i64, ()), "i": (i64, (1,))},
    "cvrp": {"current_node": (i64, (1,)), "used_capacity": (f32, (1,)), "vehicle_capacity": (f32, (1,)), "visited": (u8, ("M",))},
    "sdvrp": {"current_node": (i64, (1,)), "used_capacity": (f32, (1,)), "vehicle_capacity": (f32, (1,)),
              "demand_with_depot": (f32, ("M",))},
    "cvrptw": {"current_node": (i64, (1,)), "used_capacity": (f32, (1,)), "vehicle_capacity": (f32, (1,)),
               "visited": (u8, ("M",)), "current_time": (f32, (1,))},
    "pctsp": {"current_node": (i64, ()), "cur_total_prize": (f32, ()), "prize_required": (f32, ()), "visited": (bl, ("M",)),
              "i": (i64, ())},
    "op": {"current_node": (i64, (1,)), "tour_length": (f32, ()), "visited": (bl, ("M",)), "i": (i64, ())},
    "pdp": {"current_node": (i64, (1,)), "available": (bl, ("M",)), "to_deliver": (bl, ("M",))},
}


def rows(t, S):
    """[B, ...] -> [S B, ...] in the (s b) order of the reference's batchify."""
    return t if S <= 1 else t.repeat(S, *([1] * (t.dim() - 1)))


def storages(td):
    return {v.untyped_storage().data_ptr() for v in td.values()}


def assert_state(kind, st, want, mask, done, S, what=""):
    R, M = max(S, 1) * B, mask.shape[1]
    assert (st.env_name, st.R, st.M) == (kind, R, M)
    want = dict(want, mask=(True, bl, mask, "action_mask"), done=(True, bl, done.reshape(B), "done"))
    for slot in SLOTS + ("mask", "done"):
        got = getattr(st, slot)
        if slot not in want:
            assert got is None, f"{what}{slot} is not part of the {kind} state"
            continue
        per_row, dtype, val, _ = want[slot]
        val = rows(val, S) if per_row else val
        assert got.dtype == dtype and tuple(got.shape) == tuple(val.shape) and got.is_contiguous(), \
            f"{what}{slot}: {got.dtype} {tuple(got.shape)} contiguous={got.is_contiguous()}, want {dtype} {tuple(val.shape)}"
        assert got.shape[0] == (R if per_row else B)
        assert torch.equal(got, val.to(dtype)), f"{what}{slot}: values"


@pytest.mark.parametrize("S", [0, 2])
@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
def test_state_from_td(name, kw, S):
    from eam_rl4co_amd.policy import state_from_td

    kind = KIND.get(name, name)
    _, td = make(name, kw)
    want = expected(kind, td)
    own = storages(td)
    st = state_from_td(kind, td, S)                          # copy=True: the kernels may write into every per-row tensor
    assert_state(kind, st, want, td["action_mask"], td["done"], S)
    for slot in SLOTS + ("mask", "done"):
        if slot in ("mask", "done") or (slot in want and want[slot][0]):
            assert getattr(st, slot).untyped_storage().data_ptr() not in own, f"{slot} aliases the TensorDict"
    if S == 0:
        view = state_from_td(kind, td, 0, copy=False)
        assert_state(kind, view, want, td["action_mask"], td["done"], 0, "copy=False: ")
        for slot, (_, _, _, key) in dict(want, mask=(True, bl, None, "action_mask"), done=(True, bl, None, "done")).items():
            if key is not None:
                assert getattr(view, slot).untyped_storage().data_ptr() == td[key].untyped_storage().data_ptr(), \
                    f"copy=False: {slot} is not a view of td[{key!r}]"


@pytest.mark.parametrize("S", [0, 2])
@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
def test_state_to_td_round_trip(name, kw, S):
    from eam_rl4co_amd.policy import state_from_td, state_to_td

    kind = KIND.get(name, name)
    _, td = make(name, kw)
    R, M = max(S, 1) * B, td["action_mask"].shape[1]
    out = state_to_td(kind, state_from_td(kind, td, S), td)
    emitted = dict(EMITTED[kind], action_mask=(bl, ("M",)), done=(bl, ()), reward=(bl, ()))
    assert set(out.keys()) == set(td.keys()) | set(emitted)
    assert tuple(out.batch_size) == (R,)
    for k in out.keys():
        dtype, shape = emitted[k] if k in emitted else (td[k].dtype, tuple(td[k].shape[1:]))
        shape = tuple(M if d == "M" else d for d in shape)
        assert out[k].dtype == dtype and tuple(out[k].shape) == (R,) + shape, f"{k}: {out[k].dtype} {tuple(out[k].shape)}"
        if k == "reward":
            assert not out[k].any()
        else:
            assert torch.equal(out[k].reshape(R, -1), rows(td[k], S).reshape(R, -1)), f"{k}: values"


@pytest.mark.parametrize("name,kw", CASES[:-1], ids=IDS[:-1])       # (RolloutState has no force_start_at_depot: one pdp case)
def test_reset_state_validates(name, kw):
    from eam_rl4co_amd import ops

    kind = KIND.get(name, name)
    _, td = make(name, kw)
    M, E, R = td["action_mask"].shape[1], 128, 2 * B
    per_instance = {s: v for s, (per_row, _, v, _) in expected(kind, td).items() if not per_row}
    st = ops.RolloutState(kind, R, M, DEV, demand=per_instance.pop("demand", None))
    for slot, v in per_instance.items():                    # locs, tw, dur: the instance's own tensors
        setattr(st, slot, v.contiguous())
    buf = torch.zeros(B, M, len(ops.slot_map(kind)) * E, device=DEV)
    cvec = None if kind == "pdp" else torch.zeros(2 * E if kind == "cvrptw" else E, device=DEV)
    cache = ops.DecodeCache(kind, buf, cvec, None, None, 8, dyn=torch.zeros(3, E, device=DEV) if kind == "sdvrp" else None,
                            embed_dim=E)
    ops._validate_state(st, cache)
    assert st.struct() is not None
    assert st.mask.dtype == bl and tuple(st.mask.shape) == (R, M) and st.done.dtype == bl and not st.done.any()
    assert st.cur.dtype == i64 and not st.cur.any()
    if kind == "pdp":       # the reset state of PDPEnv: depot visited, depot and pickups open, mask = available & to_deliver
        visited = torch.zeros(R, M, dtype=u8, device=DEV)
        visited[:, 0] = 1
        to_deliver = torch.zeros(R, M, dtype=u8, device=DEV)
        to_deliver[:, :N // 2 + 1] = 1
        assert st.visited.dtype == u8 and torch.equal(st.visited, visited)
        assert st.to_deliver.dtype == u8 and torch.equal(st.to_deliver, to_deliver)
        assert torch.equal(st.mask, rows(td["action_mask"], 2)) and torch.equal(st.mask, (visited == 0) & (to_deliver != 0))
    else:
        assert st.mask.all()
    with pytest.raises(ValueError, match="state / cache shape mismatch"):
        ops._validate_state(ops.RolloutState(kind, R, M + 2, DEV), cache)


@pytest.mark.parametrize("S", [0, 2])
@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
def test_env_step_matches_env(name, kw, S):
    """One `_env_step_` on the flat state == env.step on the TensorDict, for one feasible action per row (a customer where
    one is feasible, else node 0): mask, done, current node and the env's scalars and planes."""
    from eam_rl4co_amd.policy import _env_step_, state_from_td

    kind = KIND.get(name, name)
    env, td = make(name, kw)
    mask = td["action_mask"]
    M = mask.shape[1]
    action = (mask.to(i64) * (1 + (torch.arange(M, device=DEV) > 0).to(i64))).argmax(1)
    assert mask.gather(1, action[:, None]).all()
    st = state_from_td(kind, td, S)
    _env_step_(st, rows(action, S).contiguous())
    td.set("action", action)
    nxt = env.step(td)["next"]
    assert_state(kind, st, expected(kind, nxt), nxt["action_mask"], nxt["done"], S, "after one step: ")
