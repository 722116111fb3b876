"""The PolyNet rollout-arithmetic tests' own ground, checked without a GPU: the PolyNet pointer of the yardstick (tests/rollout_ref.py,
`poly`) against tests/polynet_ref.py, which tests/test_host_polynet.py pins to the steps recorded from the reference; the
soundness of the case table (tests/polynet_cases.py: every case's conditions under its recorded seed); and the one-line mutants
of the pointer, each of which the named cases must see under exactly the checks and bounds of the GPU test
(polynet_cases.check), with the float32 restatement standing in for the kernel.

Which case catches which mutant:
  strategy of row r % k for start r // B ............... tsp_normal_M20_S16_B3_k16
  every launch of 128 starts begins at strategy 0 ...... tsp_normal_M20_S130_B3_k5, cvrp_normal_M21_S130_B3_k5 (and no other can)
  ReLU dropped ......................................... tsp_normal_M20_S16_B3_k16, cvrp_normal_M21_S16_B3_k16
  residual y = W2 h + b2 without g ..................... the same two
  b2 dropped ........................................... the same two
  the strategy table's row 0 for every row ............. the same two
  folded logit key Lp for L ............................ the same two
  glimpse over 16 ceil(M / 16) slots, last node repeated  M = 31, 33, 63, 65; M = 32 and 64 cannot show it
"""
import numpy as np
import pytest
import torch

import polynet_cases as pc
import polynet_ref as pr
import rollout_cases as rc
import rollout_ref as ref
import step_ref
from test_host_rollout_ref import cache64

E = ref.E


# ---------------------------------------------------------------------------------------------------------------------
# the pointer is polynet_ref's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["polynet_tsp20_k5_s7_greedy", "polynet_cvrp20_k8_s8_sampling"])
def test_pointer_agrees_with_polynet_ref(name):
    """Two float64 evaluations of the same expression in different association: the selected log-probs of the fixture's actions
    within 1e-10.  K / V / L / gctx are polynet_ref.cache_of's, the folds Pa / Pb / cvec come from the same weights."""
    fx, sd, want = pr.reference(name)
    env, k = str(fx["env_name"]), int(fx["k"])
    own = pr.cache_of(sd, fx["embeddings"])
    cache = cache64(sd, env, fx["embeddings"])
    cache.update({n: torch.from_numpy(own[n]) for n in ("K", "V", "L", "gctx")})
    f4 = lambda key: torch.from_numpy(np.asarray(sd["decoder.pointer." + key], np.float32))
    poly = dict(Wout=f4("project_out.weight"), W1=f4("poly_layer_1.weight"), b1=f4("poly_layer_1.bias"), W2=f4("poly_layer_2.weight"),
                b2=f4("poly_layer_2.bias"), Z=torch.from_numpy(pr.binary_vectors(k)))
    batch = pr.batch_of(fx)
    actions = np.asarray(fx["actions"])
    S = actions.shape[0] // fx["locs"].shape[0]
    op = ref.operands_of(cache, batch, actions, S)
    assert bool(op["feasible"].all()) and op["all_done"]
    if env == "cvrp":
        # the free capacity as polynet_ref forms it, a float64 difference: rollout_ref's is the reference's own float32 one (pinned
        # by tests/test_host_rollout_ref.py), 6e-8 away -- 4e-9 on a log-prob, which is not the pointer's association
        hist = step_ref.replay(batch, actions, S)
        op["sc"] = torch.tensor([[np.float64(s["vcap"]) - np.float64(s["used"]) for s in hist[t]] for t in range(actions.shape[1])]).T[None]
    got = ref.run(op, torch.float64, poly=poly)["logp"].numpy().copy()
    if bool(fx["forced_start"]):
        got[:, 0] = 0.0                 # (the start node of a multistart rollout is no decision)
    err = float(np.abs(got - want).max())
    print(f"{name}: {err:.3e} from polynet_ref over {got.size} log-probs, |logp| up to {np.abs(want).max():.2f}")
    assert np.abs(want).max() > 1.0
    assert err <= 1e-10


def test_without_the_pointer_nothing_changes():
    """poly=None: `run` returns what it returned, bit for bit, whether or not the cache carries L."""
    c, batch, cch, q = rc.operands("cvrp_normal_M21_S4")
    actions, _ = ref.rollout(cch, batch, c["S"], "greedy", None, torch.float32)
    plain = ref.run(ref.operands_of(cch, batch, actions.numpy(), c["S"]), torch.float32, rowwise=True)
    with_l = ref.run(ref.operands_of(dict(cch, L=torch.randn_like(cch["K"])), batch, actions.numpy(), c["S"]), torch.float32, rowwise=True)
    assert set(plain) == set(with_l) == {"logp", "lse", "u", "logp_all", "heads"}
    for key in plain:
        assert torch.equal(plain[key], with_l[key]), key


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def test_case_table_is_the_one_promised():
    cases = list(pc.CASES.values())
    of = lambda env, **kw: {c["M"] for c in cases if c["env"] == env and all(c[a] == b for a, b in kw.items())}
    for kind in ("policy", "normal"):
        assert of("tsp", kind=kind) == {2, 20, 31, 32, 33, 63, 64, 65, 100, 112} and of("cvrp", kind=kind) == {21, 32, 33, 64, 65, 112}
    for kind in ("peaked", "clip0", "temp0.5", "temp2", "saturated"):
        assert of("tsp", kind=kind) == {20, 33, 65} and of("cvrp", kind=kind) == {21, 33, 65}
    assert of("tsp", kind="tie") == {20, 33, 65, 112} and of("cvrp", kind="tie") == {21, 33, 65, 112}
    shapes = {(c["S"], c["B"]) for c in cases}
    assert shapes >= {(2, 3), (16, 3), (17, 3), (40, 100), (17, 129), (128, 1), (130, 3)}
    assert {c["env"] for c in cases if c["S"] == 130} == {"tsp", "cvrp"}
    assert {c["k"] for c in cases} == {1, 2, 5, 16, 128} and any(c["k"] > c["S"] for c in cases)
    assert all(c["M"] == 20 + (c["env"] == "cvrp") for c in cases if c["S"] >= 128 or c["B"] > 3)
    assert len(cases) == 76 and set(pc.PER_TILE_COUNT) <= set(pc.CASES) and set(pc.SEEDS) | set(pc.SATURATED) <= set(pc.CASES)
    assert {(c["env"], 2 if c["M"] <= 32 else 4 if c["M"] <= 64 else 7) for c in map(pc.CASES.get, pc.PER_TILE_COUNT)} == \
        {(env, n) for env in ("tsp", "cvrp") for n in (2, 4, 7)}


@pytest.mark.parametrize("name", [n for n in pc.NAMES if pc.CASES[n]["kind"] == "tie"])
def test_twins_are_bit_identical_in_every_operand(name):
    c, batch, cache, q = pc.operands(name)
    assert rc.twins(c)
    for lo, hi in rc.twins(c):
        for k in ("K", "V", "L", "Lp", "Pa", "Pb"):
            assert cache[k] is None or torch.equal(cache[k][:, lo], cache[k][:, hi]), k
        assert torch.equal(q[..., lo], q[..., hi])


def test_the_fold_is_the_fold_of_L():
    _, _, cache, _ = pc.operands("tsp_normal_M20_S16_B3_k16")
    want = cache["L"].double() @ cache["poly"]["Wout"].double()
    assert float((cache["Lp"].double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


def test_the_last_two_starts_of_the_split_cvrp_case_are_the_slowest():
    """On the restatement's own float64 sampling rollout: the slowest row of the first 128 starts needs fewer steps than the slowest
    of the last two, so a final state padded against the first launch's step count differs from the reference's."""
    name = "cvrp_normal_M21_S130_B3_k5"
    c, batch, cch, q = pc.operands(name)
    actions, _ = pc.reference_rollout(c, batch, cch, q, "sampling")
    op = ref.operands_of(cch, batch, actions.numpy(), c["S"])
    steps = (~op["done"]).sum(1)
    first, last = int(steps[:128 * c["B"]].max()), int(steps[128 * c["B"]:].max())
    print(f"{name}: the slowest of the first 128 starts takes {first} steps, of the last two {last}")
    assert op["all_done"] and first < last
    # ... and some row of the first launch ends its own launch on a customer: the row a premature padding leaves there
    ends = actions[:128 * c["B"], first - 1]
    assert bool((ends != 0).any())


# ---------------------------------------------------------------------------------------------------------------------
# the checks see every mutant, and pass the float32 restatement
# ---------------------------------------------------------------------------------------------------------------------
def stand_in(name, mode, mutant=None):
    """The float32 restatement as the kernel (test_host_rollout_ref.stand_in): its decode loop chooses the tour; the log-probs
    it reports are its own float32 evaluation of that tour in one batch, with the same mutant."""
    c, batch, cache, q = pc.operands(name)
    clip, temp = pc.clip_temp(c)
    actions, logps = ref.rollout(cache, batch, c["S"], mode, q, torch.float32, clip, temp, pc.t_max(c), mutant)
    op = ref.operands_of(cache, batch, actions.numpy(), c["S"], 0, clip, temp)
    if bool(op["feasible"].all()):
        logps = ref.run(op, torch.float32, mutant)["logp"]
    return actions, logps


@pytest.mark.parametrize("name", pc.NAMES)
def test_case_meets_its_conditions_and_passes_the_float32_restatement(name):
    c, batch, cache, q = pc.operands(name)
    fig, fails = pc.conditions(c, batch, cache, q)
    print(f"{name} (weight seed {pc.SEEDS.get(name, 0)}): " + ", ".join(f"{a} {b:.3e}" for a, b in fig.items() if b is not None))
    assert fails == []
    for mode in pc.MODES:
        actions, logps = stand_in(name, mode)
        assert pc.check(name, mode, actions, logps)["misses"] == [], mode


BOTH = ("tsp_normal_M20_S16_B3_k16", "cvrp_normal_M21_S16_B3_k16")
SEEN_BY = [("strategy_of_r_mod_k", "tsp_normal_M20_S16_B3_k16")] + [("s_first_ignored", n) for n in pc.SPLIT] + \
    [(m, n) for m in ("relu_dropped", "residual_g_dropped", "b2_dropped", "ctab_of_strategy_0", "folded_Lp_for_L") for n in BOTH] + \
    [("padded_slots_not_zero", n) for n in pc.NAMES if pc.CASES[n]["M"] in (31, 33, 63, 65) and pc.CASES[n]["kind"] in ("policy", "normal")]


@pytest.mark.parametrize("mutant,name", SEEN_BY)
def test_case_table_sees_the_mutant(mutant, name):
    assert {m for m, _ in SEEN_BY} == set(ref.POLY_MUTANTS)
    for mode in pc.MODES:
        actions, logps = stand_in(name, mode, mutant)
        misses = pc.check(name, mode, actions, logps)["misses"]
        assert misses, (mutant, name, mode)


@pytest.mark.parametrize("name", [n for n in pc.NAMES if pc.CASES[n]["M"] in (32, 64) and pc.CASES[n]["kind"] == "normal"])
def test_whole_key_tiles_have_no_padded_slots(name):
    for mode in pc.MODES:
        a0, l0 = stand_in(name, mode)
        a1, l1 = stand_in(name, mode, "padded_slots_not_zero")
        assert torch.equal(a0, a1) and torch.equal(l0, l1)


def test_only_a_split_rollout_shows_an_ignored_first_start():
    assert pc.SPLIT == ["tsp_normal_M20_S130_B3_k5", "cvrp_normal_M21_S130_B3_k5"]
    name = "tsp_normal_M20_S128_B1_k128"
    a0, l0 = stand_in(name, "greedy")
    a1, l1 = stand_in(name, "greedy", "s_first_ignored")
    assert torch.equal(a0, a1) and torch.equal(l0, l1)
