"""env_spec.ENV_SPECS against the package's own envs (reset on the CPU) and against the literals the table replaced."""
import pytest

from eam_rl4co_amd import _lib, env_spec
from eam_rl4co_amd.env_spec import ENV_SPECS, dims, spec

B, N = 3, 6
CASES = [("tsp", {}), ("cvrp", {}), ("sdvrp", {}), ("cvrptw", {}), ("pctsp", {}), ("spctsp", {}), ("op", {}), ("pdp", {}),
         ("pdp", {"force_start_at_depot": True})]
IDS = [n + ("-depot" if kw else "") for n, kw in CASES]
FAMILIES = ("tsp", "cvrp", "sdvrp", "pctsp", "op", "cvrptw", "pdp")


def td_keys(args):
    """The TensorDict keys among the arguments of a `reward` / `check` entry (not "<pseudo>", not "=literal")."""
    return tuple(a for a in args if isinstance(a, str) and a[0] not in "<=")


@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
def test_record_matches_the_env(name, kw):
    import eam_rl4co_amd as ea

    td = ea.get_env(name, generator_params=dict(num_loc=N), **kw).reset(batch_size=[B])
    rec = spec(name)
    M = td["action_mask"].shape[1]
    for key in td_keys(rec.reward[1]) + td_keys(rec.check[1]) + rec.reeval_static:
        assert key in td.keys(), f"{name}: the record names td[{key!r}], which the env does not have"
    for f in rec.fields:
        assert f.key in td.keys(), f"{name}: {f.slot} comes from td[{f.key!r}], which the env does not have"
        t = td[f.key]
        assert t.dtype == (f.src_dtype or f.dtype), f"{name}: td[{f.key!r}] is {t.dtype}"
        if f.transform == "col0":
            t = t[..., 0]
        else:
            assert f.transform in (None, "not")
        assert tuple(t.shape) == (B,) + dims(f.shape, M), f"{name}: td[{f.key!r}] is {tuple(t.shape)}"
        assert f.meaning and f.reset in ("zeros", "ones", "depot", "depot_and_pickups")
    slots = [f.slot for f in rec.fields]
    for slot, _ in _lib.State._fields_:
        if slot in ("mask", "done", "heads_out"):
            assert slot not in slots
        else:
            assert slots.count(slot) <= 1, f"{name}: two fields claim {slot}"
    assert set(slots) <= {s for s, _ in _lib.State._fields_}
    # the step wrapper's arguments are slots the env has (or the common mask / done, the action, nothing)
    assert all(a in (None, env_spec.ACTION, "mask", "done") or a in slots for a in rec.step[1])


def test_families_aliases_and_abi_ids():
    from eam_rl4co_amd import ops
    from eam_rl4co_amd.policy import _kind

    assert tuple(sorted(ENV_SPECS)) == tuple(sorted(FAMILIES)) and all(k == v.name for k, v in ENV_SPECS.items())
    assert env_spec.ALIASES == {"spctsp": "pctsp"}
    assert _kind("spctsp") == "pctsp" and _kind("op") == "op" and spec("spctsp") is ENV_SPECS["pctsp"]
    assert ops.ENVS == {"tsp": _lib.ENV_TSP, "cvrp": _lib.ENV_CVRP, "sdvrp": _lib.ENV_SDVRP, "pctsp": _lib.ENV_PCTSP,
                        "op": _lib.ENV_OP, "cvrptw": _lib.ENV_CVRPTW, "pdp": _lib.ENV_PDP}


def test_state_columns():
    assert {n: s.n_state_cols for n, s in ENV_SPECS.items()} == {"tsp": 0, "cvrp": 1, "sdvrp": 1, "pctsp": 1, "op": 1,
                                                                 "cvrptw": 2, "pdp": 0}


def test_check_messages():
    want = {"tsp": ("Invalid tour", "Used more than capacity"), "cvrp": ("Invalid tour", "Used more than capacity"),
            "cvrptw": ("Invalid tour", "Used more than capacity"),
            "sdvrp": ("All demand must be satisfied", "Cannot visit depot twice if any nonzero demand"),
            "pctsp": ("Duplicates", "Total prize does not satisfy min total prize"),
            "op": ("Duplicates", "Max length exceeded"),
            "pdp": ("Not visiting all nodes", "Deliverying without pick-up")}
    assert {n: s.messages for n, s in ENV_SPECS.items()} == want
    assert {n: s.check_padded for n, s in ENV_SPECS.items()} == {"tsp": "if_full", "cvrp": "yes", "sdvrp": "no",
                                                                    "pctsp": "yes", "op": "yes", "cvrptw": "no", "pdp": "yes"}


def test_native_envs_are_recognised_by_class():
    """`_enqueue` takes its fast path for the package's own env classes only: a subclass may override reward or checks."""
    from eam_rl4co_amd import envs

    class MyTSP(envs.TSPEnv):
        pass

    assert all(type(envs.get_env(n, generator_params=dict(num_loc=N))) in envs.ENV_REGISTRY.values()
               for n in envs.ENV_REGISTRY)
    assert type(MyTSP(generator_params=dict(num_loc=N))) not in envs.ENV_REGISTRY.values()
