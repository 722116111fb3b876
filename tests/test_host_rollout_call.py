"""No GPU -- and ONLY without one: argument validation of the five whole-rollout entry points (eamrl_am_rollout, _seeded, _polynet,
_polynet_seeded, _eas_layer), which share one call path (rollout_call in csrc/abi.hip; DESIGN.md "The whole-rollout call path").

The module skips itself where torch.cuda.is_available().  The cases (tests/rollout_call_cases.py) are one-fault-at-a-time edits of
an otherwise valid call on hand-built structs with made-up addresses, so a requirement that got lost would launch a kernel on
those addresses; without a device such a launch fails at once with EAMRL_E_LAUNCH, which is also what the valid calls return.

Every case's return code is compared with tests/golden/rollout_call_errors.json, recorded from the library as it was before the
entry points shared their call path (tests/golden/make_golden_rollout_call.py), and the message must name the function that was
called.  The same file holds that build's answers of the four host-only shape queries.  `ops._rollout_inputs`, the one
normalisation of (noise, given, t_max) behind ops.rollout, is checked against values worked out by hand from the three copies it
replaced.
"""
import json
import os

import pytest
import torch

import rollout_call_cases as cc

if torch.cuda.is_available():
    pytest.skip("one-fault-at-a-time calls on made-up addresses: a lost requirement would launch on them", allow_module_level=True)

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_call_errors.json")) as f:
    GOLDEN = json.load(f)
CASES = cc.cases()


def test_the_golden_file_holds_exactly_the_cases():
    assert set(GOLDEN["codes"]) == {c[0] for c in CASES}
    for cid, _, _, _, breaks in CASES:
        # a broken requirement is EAMRL_E_ARG; a valid call gets as far as the launch
        assert GOLDEN["codes"][cid] == (cc.E_ARG if breaks else cc.E_LAUNCH), cid
    # what the recorded build answered differently: it filled the noise scratch (a launch) before it rejected these two
    assert sorted(GOLDEN["let_through"]) == ["eamrl_am_rollout_seeded/pdp/state_to_deliver_null",
                                             "eamrl_am_rollout_seeded/pdp/state_visited_null"]


def test_every_entry_point_and_env_has_its_cases():
    seen = {(entry, env) for _, entry, env, _, _ in CASES}
    assert seen == {(entry, env) for entry, envs in cc.ENTRIES.items() for env in envs}
    names = {cid.split("/")[2] for cid, entry, _, _, _ in CASES if entry == "eamrl_am_rollout_eas_layer"}
    assert {"rows_per_instance_1", "rows_per_instance_129", "M_113", "env_pctsp", "layer_forced_without_t_forced"} <= names


@pytest.mark.parametrize("cid,entry,env,call,breaks", CASES, ids=[c[0] for c in CASES])
def test_return_code_and_message_prefix(cid, entry, env, call, breaks):
    rc, msg = cc.invoke(call)
    assert rc == GOLDEN["codes"][cid], f"{cid}: {rc} ({msg})"
    assert msg.split(":")[0] == entry, f"{cid}: the message does not name the called function: {msg!r}"


def test_shape_queries_answer_as_recorded():
    got = cc.predicates()
    assert set(got) == set(GOLDEN["predicates"])
    wrong = {k: (v, GOLDEN["predicates"][k]) for k, v in got.items() if v != GOLDEN["predicates"][k]}
    assert not wrong


# (noise shape, given shape, t_max, env) -> (t_max, t_given); R = 6 rows, M = 10 nodes.  By hand from the rules the three former
# copies shared: a noise tensor sets t_max to its own step count, longer or shorter; given actions set t_given and, without
# noise, bound t_max on every env but TSP (whose tours have one length).
R, M = 6, 10
TABLE = [
    (None, None, 21, "cvrp", (21, 0)),
    ((R, 15, M), None, 21, "cvrp", (15, 0)),
    ((R, 30, M), None, 21, "cvrp", (30, 0)),
    (None, (R, 7), 21, "cvrp", (7, 7)),
    (None, (R, 7), 9, "tsp", (9, 7)),
    (None, (R, 30), 21, "cvrp", (21, 30)),
    (None, (R, 7), 21, "pctsp", (7, 7)),
    ((R, 15, M), (R, 7), 21, "cvrp", (15, 7)),
    ((R, 9, M), (R, 7), 21, "tsp", (9, 7)),
]
BAD = [
    ((R + 1, 15, M), None, ValueError, r"noise must be \[R, T, M\]"),
    ((R, 15, M + 1), None, ValueError, r"noise must be \[R, T, M\]"),
    ((R, M), None, ValueError, r"noise must be \[R, T, M\]"),           # not 3-D: the same error on every path
    (None, (R,), ValueError, r"given actions must be \[R, T\]"),
    (None, (R + 1, 7), ValueError, r"given actions must be \[R, T\]"),
]


@pytest.fixture
def host_ops(monkeypatch):
    """ops with the device check of its tensor arguments switched off: the helper reads shapes and dtypes only."""
    from eam_rl4co_amd import ops

    monkeypatch.setattr(ops, "_need_gpu", lambda t, name: None)
    return ops


@pytest.mark.parametrize("noise,given,t_max,env,want", TABLE)
def test_rollout_inputs_table(host_ops, noise, given, t_max, env, want):
    n = None if noise is None else torch.zeros(noise)
    g = None if given is None else torch.zeros(given, dtype=torch.int64)
    n2, g2, t, tg = host_ops._rollout_inputs(n, g, t_max, env, R, M)
    assert n2 is n and g2 is g and (t, tg) == want and type(t) is int


@pytest.mark.parametrize("noise,given,exc,match", BAD)
def test_rollout_inputs_rejects(host_ops, noise, given, exc, match):
    n = None if noise is None else torch.zeros(noise)
    g = None if given is None else torch.zeros(given, dtype=torch.int64)
    with pytest.raises(exc, match=match):
        host_ops._rollout_inputs(n, g, 21, "cvrp", R, M)
    with pytest.raises(TypeError):
        host_ops._rollout_inputs(torch.zeros(R, 15, M, dtype=torch.float64), None, 21, "cvrp", R, M)
    with pytest.raises(TypeError):
        host_ops._rollout_inputs(None, torch.zeros(R, 7, dtype=torch.int32), 21, "cvrp", R, M)
