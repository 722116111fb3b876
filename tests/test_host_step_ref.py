"""Host: tests/step_ref.py -- the plain float32 restatement of every env's step-and-mask rule -- against states recorded from
the unmodified reference envs: the boundary cases of tests/step_cases.py (step_boundary.npz, written by
tests/golden/make_golden_step.py) and the random feasible walks (env_*_random.npz).  Masks, `done`, integer state and
float32 state are compared bit for bit.  The verdict each boundary case claims is asserted on the RECORDED data, so a
case whose value rounded the wrong way fails here and not on the GPU."""
import numpy as np
import pytest

import step_cases
import step_ref
from _util import golden
from eam_rl4co_amd import env_spec

RANDOM_WALKS = ["env_tsp20_random", "env_cvrp20_random", "env_cvrp100_random", "env_sdvrp20_random", "env_pctsp20_random",
                "env_spctsp20_random", "env_op20_random", "env_op50_random", "env_cvrptw20_random", "env_cvrptw50_random",
                "env_pdp20_random"]
# bookkeeping of the reference's step besides the slots of env_spec: TensorDict key -> step_ref's name
EXTRA_KEYS = {"current_total_prize": "prize_tot"}


def recorded_keys(env_name):
    """TensorDict key -> (step_ref slot, transform) for the per-row state of an env."""
    out = {f.key: (f.slot, f.transform) for f in env_spec.spec(env_name).fields if f.per_row and f.emit}
    out.update({k: (v, None) for k, v in EXTRA_KEYS.items()})
    return out


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and b.dtype == np.float32 and bool((a.view(np.uint32) == b.view(np.uint32)).all())
    return a.shape == b.shape and bool((a == b).all())


def assert_states_equal(fx, prefix, sel, states, env_name, what):
    """The recorded tensors `prefix + key` (at `sel`) against a list of step_ref states."""
    mask = np.stack([s["mask"] for s in states])
    assert same_bits(fx[prefix + "action_mask"][sel], mask), f"{what}: mask"
    if prefix + "done" in fx:
        done = np.array([s["done"] for s in states])
        assert same_bits(fx[prefix + "done"][sel].reshape(done.shape), done), f"{what}: done"
    compared = []
    for key, (slot, transform) in recorded_keys(env_name).items():
        if prefix + key not in fx:
            continue
        rec = fx[prefix + key][sel]
        got = np.stack([np.asarray(s[slot]) for s in states])
        if transform == "not":
            got = got == 0
        got = got.astype(rec.dtype).reshape(rec.shape)
        assert same_bits(rec, got), f"{what}: {key}: {rec.tolist()} vs {got.tolist()}"
        compared.append(key)
    return compared


def check_against_recording(fx, batch, env_name, what):
    actions = fx["step_action"]
    hist = step_ref.replay(batch, actions)
    compared = assert_states_equal(fx, "reset_", slice(None), hist[0], env_name, f"{what} reset")
    for t in range(actions.shape[1]):
        compared = assert_states_equal(fx, "step_", (slice(None), t), hist[t + 1], env_name, f"{what} step {t}")
    want = {f.key for f in env_spec.spec(env_name).fields if f.per_row and f.emit and f.slot != "vcap"}
    assert want <= set(compared), f"{what}: state tensors not recorded: {want - set(compared)}"
    for t, states in enumerate(hist):       # (bookkeeping no decision reads: torch sums the penalties pairwise at reset)
        if "step_cur_total_penalty" in fx and t > 0:
            np.testing.assert_allclose([s["pen_tot"] for s in states], fx["step_cur_total_penalty"][:, t - 1], rtol=1e-6)
    return hist


def boundary(name):
    fx = golden("step_boundary")
    return {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + "/")}


def test_fixture_set_is_complete():
    """Every named case of step_cases is in the fixture, with the inputs the case has today, and none is empty."""
    names = [c["name"] for c in step_cases.named_cases()]
    assert names == step_cases.NAMES and len(set(names)) == len(names)
    assert list(golden("step_boundary")["names"]) == names
    assert {env_spec.spec(c["env"]).name for c in step_cases.named_cases()} == set(env_spec.ENV_SPECS)
    for case in step_cases.named_cases():
        fx = boundary(case["name"])
        assert str(fx["env_name"]) == case["env"] and fx["step_action"].shape[0] == 3 and fx["step_action"].shape[1] >= 2
        for k, v in case["batch"].items():
            if k != "env":
                assert same_bits(fx["in_" + k], np.asarray(v)), f"{case['name']}: input {k} differs from the recorded one"
        assert case["verdicts"], case["name"]


@pytest.mark.parametrize("name", step_cases.NAMES)
def test_step_ref_reproduces_the_recorded_boundary_states(name):
    case = step_cases.case_by_name(name)
    fx = boundary(name)
    check_against_recording(fx, case["batch"], case["env"], name)
    if case["env"] == "op":     # reset's arithmetic: the arrival limit per node
        limits = np.stack([s["demand"] for s in step_ref.reset_rows(case["batch"])])
        assert same_bits(fx["reset_max_length"], limits)


@pytest.mark.parametrize("name", RANDOM_WALKS)
def test_step_ref_reproduces_the_recorded_random_walks(name):
    fx = golden(name)
    batch = {k[4:]: v for k, v in fx.items() if k.startswith("gen_")}
    batch["env"] = str(fx["env_name"])
    check_against_recording(fx, batch, batch["env"], name)


@pytest.mark.parametrize("name", ["env_op20_random", "env_op50_random", "env_cvrptw20_random", "env_cvrptw50_random"])
def test_leg_formula_is_the_one_the_reference_uses(name, monkeypatch):
    """sqrt(fma(dy, dy, dx * dx)) reproduces every recorded tour length / clock; the three other candidates do not (over
    the four fixtures together: a single walk can miss the few legs on which two formulas differ)."""
    fx = golden(name)
    batch = {k[4:]: v for k, v in fx.items() if k.startswith("gen_")}
    batch["env"] = str(fx["env_name"])
    key, slot = ("step_tour_length", "used") if batch["env"] == "op" else ("step_current_time", "time")
    wrong = {}
    for formula in step_ref.LEG_FORMULAS:
        monkeypatch.setattr(step_ref, "LEG", formula)
        hist = step_ref.replay(batch, fx["step_action"])
        got = np.stack([[s[slot] for s in states] for states in hist[1:]], 1).astype(np.float32)
        wrong[formula] = int((got.view(np.uint32) != fx[key].reshape(got.shape).view(np.uint32)).sum())
    assert wrong["fma_y"] == 0, wrong
    if name == "env_op20_random":
        assert all(wrong[f] > 0 for f in ("fma_x", "plain", "float64")), wrong


@pytest.mark.parametrize("name", step_cases.NAMES)
def test_boundary_verdicts_hold_in_the_reference(name):
    """What each case claims -- feasible at the boundary, infeasible one float32 step above, done or not, the exact value of a
    slot -- read off the reference's recorded tensors."""
    case = step_cases.case_by_name(name)
    fx = boundary(name)
    keys = {slot: (key, tr) for key, (slot, tr) in recorded_keys(case["env"]).items()}
    T = fx["step_action"].shape[1]
    for b, t, kind, arg, expected, label in case["verdicts"]:
        assert 0 <= t <= T, f"{name}: '{label}' names step {t} of {T}"
        pre, sel = ("reset_", b) if t == 0 else ("step_", (b, t - 1))
        if kind == "mask":
            got = fx[pre + "action_mask"][sel][arg]
        elif kind == "done":
            got = fx[pre + "done"][sel].reshape(())
        else:
            got = fx[pre + keys[arg][0]][sel].reshape(())
        if isinstance(expected, np.float32):
            assert got.dtype == np.float32 and got.view(np.uint32) == expected.view(np.uint32), f"{name}: {label}: {got!r}"
        else:
            assert got == expected, f"{name}: {label}: instance {b} after {t} steps: {got!r}, claimed {expected!r}"


@pytest.mark.parametrize("name", step_cases.NAMES)
def test_no_reachable_state_has_an_empty_mask(name):
    """On the recorded reference run, and on step_ref's runs with four starts per instance (rows whose seeded tails differ)."""
    case = step_cases.case_by_name(name)
    fx = boundary(name)
    done = np.concatenate([fx["reset_done"].reshape(3, 1), fx["step_done"].reshape(3, -1)], 1)
    masks = np.concatenate([fx["reset_action_mask"][:, None], fx["step_action_mask"]], 1)
    live = ~done if case["env"] in ("pdp", "tsp") else np.ones_like(done)     # (PDP / TSP: a finished row has no node left)
    assert masks.any(-1)[live].all()
    for S in (1, 4):
        actions, counts, final, _ = step_ref.rollout_first_feasible(case["batch"], step_cases.prefs(case, S))
        assert (counts >= 1).all() and all(s["done"] for s in final)
        if S == 1:
            assert same_bits(actions, fx["step_action"]), "first-feasible rollout vs the reference driven the same way"


def row_lengths(name):
    done = boundary(name)["step_done"].reshape(3, -1)
    return (np.cumsum(done, 1) == 0).sum(1) + 1


@pytest.mark.parametrize("env_name", ["cvrp", "cvrptw", "sdvrp", "pctsp", "spctsp", "op"])
def test_some_row_finishes_several_steps_before_the_others(env_name):
    """... so that the padding of finished rows is exercised (TSP and PDP rows all take the same number of steps)."""
    spread = {c["name"]: row_lengths(c["name"]) for c in step_cases.named_cases() if c["env"] == env_name}
    assert any(v.max() - v.min() >= 2 for v in spread.values()), spread


@pytest.mark.parametrize("env_name", ["cvrp", "cvrptw", "sdvrp", "pctsp", "op", "pdp"])
def test_padded_variants_keep_the_boundary_steps(env_name):
    """padded(case, M): the rows' first steps are the named case's, under the node map; every state has a feasible action."""
    M = 65
    for case in [c for c in step_cases.named_cases() if c["env"] == env_name]:
        big = step_cases.padded(case, M)
        actions, counts, final, _ = step_ref.rollout_first_feasible(big["batch"], step_cases.prefs(big, 1))
        assert (counts >= 1).all() and all(s["done"] for s in final)
        if env_name == "pdp":
            continue
        nm = step_cases.node_map(case["M"], M)
        small = boundary(case["name"])["step_action"]
        n_heads = min(len(h) for h in case["heads"])
        assert same_bits(actions[:, :n_heads], nm[small[:, :n_heads]]), case["name"]
