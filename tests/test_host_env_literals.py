"""Literals of the per-env host tables as they were before eam_rl4co_amd/env_spec.py existed: this file imports nothing of
the table, so it runs unchanged on the code the table replaced."""
import pytest
import torch

from eam_rl4co_amd import _lib

FAMILIES = ("tsp", "cvrp", "sdvrp", "pctsp", "op", "cvrptw", "pdp")


def test_slot_map_and_abi_ids():
    from eam_rl4co_amd import ops

    assert ops.slot_map("tsp") == {"K": 0, "V": 1, "L": 2, "Pa": 3, "Pb": 4, "Lp": 5}
    for name in FAMILIES[1:]:
        assert ops.slot_map(name) == {"K": 0, "V": 1, "L": 2, "Pa": 3, "Lp": 4}
    assert ops.ENVS == {"tsp": 0, "cvrp": 1, "sdvrp": 2, "pctsp": 3, "op": 4, "cvrptw": 5, "pdp": 6}


@pytest.mark.parametrize("M", [3, 7, 21])
def test_max_decode_steps(M, monkeypatch):
    from eam_rl4co_amd import ops
    from eam_rl4co_amd.policy import _max_decode_steps

    for npre in (0, 1):
        want = {"tsp": M - npre, "cvrp": 2 * M + 1, "sdvrp": 3 * M + 1, "pctsp": M + 1, "op": M + 1, "cvrptw": 2 * M + 1,
                "pdp": M - npre}
        assert {n: _max_decode_steps(n, M, npre) for n in FAMILIES} == want

    # ops.rollout's default t_max is the same bound: read it off the size of the outputs it allocates
    class Stop(Exception):
        pass

    def outputs(R, t_max, dev):
        raise Stop(t_max)

    monkeypatch.setattr(ops, "_validate_state", lambda st, cache: None)
    monkeypatch.setattr(ops, "_rollout_outputs", outputs)
    monkeypatch.setattr(_lib, "load", lambda: None)
    for name in FAMILIES:
        st = ops.RolloutState(name, 2, M, "cpu")
        st.mask = torch.ones(2, M, dtype=torch.bool)
        with pytest.raises(Stop) as e:
            ops.rollout(st, None, "greedy")
        assert e.value.args[0] == _max_decode_steps(name, M, 0), name


def test_reeval_static_keys():
    from eam_rl4co_amd import train

    assert train._STATE_KEYS == {"cvrp": ("demand", "vehicle_capacity"), "sdvrp": ("demand", "vehicle_capacity"),
                                 "cvrptw": ("demand", "vehicle_capacity", "locs", "time_windows", "durations"),
                                 "op": ("locs", "max_length"), "pctsp": ("real_prize", "prize_required"), "tsp": (),
                                 "pdp": ("available", "to_deliver", "action_mask")}
