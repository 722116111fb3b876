"""The rollout-arithmetic tests' own ground, checked without a GPU: the yardstick (tests/rollout_ref.py) against the per-step
log-probs and masks recorded from the reference, the soundness of the case table (tests/rollout_cases.py), and the one-line
mutants of the yardstick, each of which the named case must see under exactly the checks and bounds of the GPU test
(rollout_cases.check), with the float32 restatement standing in for a kernel.

Which case catches which mutant:
  mask on the logits but not on the glimpse ............ tsp_normal_M20_S1
  instance r // S for r % B ............................ cvrp_normal_M21_S4
  rem of step t - 1 used at step t ..................... none can: see tests/rollout_ref.py and the test below
  rem never updated .................................... sdvrp_peaked_M21_S4
  state column dropped ................................. cvrp_normal_M21_S1, cvrptw_normal_M21_S1 (the clock)
  state column of step t - 1 used at step t ............ cvrp_normal_M21_S1
  TSP placeholder step ignored ......................... tsp_normal_M20_S1
  first and current node swapped ....................... tsp_normal_M20_S1
  temperature before the clip .......................... tsp_temp0.5_M20_S1
  mask before the clip ................................. cvrp_normal_M21_S1
  sampling key logp - noise ............................ tsp_normal_M20_S1 (sampling)
  a tie goes to the higher index ....................... tsp_tie_M20_S1, cvrp_saturated_M21_S1
"""
import numpy as np
import pytest
import torch

import pdp_ref
import rollout_cases as rc
import rollout_ref as ref
import step_ref
from _util import golden, golden_weights

E = ref.E
FIXTURES = ["tsp20_greedy", "cvrp20_greedy", "sdvrp20_greedy", "pctsp20_greedy", "op20_greedy", "cvrptw20_greedy", "pdp20_greedy"]


# ---------------------------------------------------------------------------------------------------------------------
# the query mapping is the reference's
# ---------------------------------------------------------------------------------------------------------------------
def cache64(sd, env, emb):
    """The decoder cache in float64 from the weights and the node embeddings: K, V, L = the thirds of project_node_embeddings;
    the folds of DESIGN.md, Pa / Pb = emb times the node halves of project_context, Lp = L times project_out; cvec = the
    state columns of project_context (TSP: project_context(W_placeholder)); dyn = the thirds of the dynamic embedding's
    projection, the logit third folded like Lp."""
    f8 = lambda k: torch.from_numpy(np.asarray(sd[k], np.float64))
    emb = torch.from_numpy(np.asarray(emb, np.float64))
    Wkvl, Wctx, Wout = f8("decoder.project_node_embeddings.weight"), f8("decoder.context_embedding.project_context.weight"), \
        f8("decoder.pointer.project_out.weight")
    K, V, L = (emb @ Wkvl[i * E:(i + 1) * E].T for i in range(3))
    out = dict(K=K, V=V, Lp=L @ Wout, Pa=emb @ Wctx[:, :E].T, Pb=None, Cvec=None, dyn=None,
               gctx=emb.mean(1) @ f8("decoder.project_fixed_context.weight").T)
    if env == "tsp":
        out["Pb"] = emb @ Wctx[:, E:2 * E].T
        out["Cvec"] = (Wctx @ f8("decoder.context_embedding.W_placeholder"))[None]
    elif Wctx.shape[1] > E:
        out["Cvec"] = Wctx[:, E:].T.contiguous()
    if env == "sdvrp":
        wk, wv, wl = f8("decoder.dynamic_embedding.projection.weight")[:, 0].reshape(3, E)
        out["dyn"] = torch.stack([wk, wv, wl @ Wout])
    return out


def batch_of(fx):
    env = str(fx["env_name"])
    if env == "tsp":
        return {"env": env, "locs": fx["locs"]}
    batch = {"env": env, "depot": fx["locs"][:, 0], "locs": fx["locs"][:, 1:]}
    for k in ("demand", "time_windows", "durations"):
        if k in fx:
            batch[k] = fx[k]
    if env == "pctsp":
        assert (fx["prize_required"] == 1).all() and not fx["real_prize"][:, 0].any()
        batch.update(deterministic_prize=fx["real_prize"][:, 1:], stochastic_prize=fx["real_prize"][:, 1:], penalty=fx["penalty"][:, 1:])
    if env == "op":     # the fixture holds the arrival limits of the reset; the length limit itself is limit[0] + 1e-6
        batch["prize"] = fx["prize"][:, 1:]
        batch["max_length"] = (fx["max_length"][:, 0] + np.float32(1e-6)).astype(np.float32)
    if "vehicle_capacity" in fx:
        assert (fx["vehicle_capacity"] == 1).all()
    return batch


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_recorded_reference_steps(name, oracle):
    """The yardstick's full log-prob vectors along the fixture's actions against the recorded ones, at the feasible entries, with
    the tolerance tests/test_oracle_golden.py applies to these arrays; its masks against the recorded masks, exactly."""
    fx = golden(name)
    env = str(fx["env_name"])
    if env == "pdp":
        sd = pdp_ref.weights(pdp_ref.cfg_for(fx))
        emb = pdp_ref.encode(sd, fx["locs"])[1]
    else:
        sd, emb = golden_weights("am_" + env), fx["embeddings"]
    cache = cache64(sd, env, emb)
    if "graph_context" in fx:
        np.testing.assert_allclose(cache["gctx"].numpy(), fx["graph_context"], rtol=0, atol=2e-4 * float(np.abs(fx["graph_context"]).max())
                                   if env == "cvrptw" else 1e-5)
    batch = batch_of(fx)
    start = None
    if env == "op":      # the arrival limits as recorded, not as recomputed from the rounded length limit
        start = step_ref.reset_rows(batch)
        for b, s in enumerate(start):
            s["demand"], s["vcap"] = fx["max_length"][b].astype(np.float32), np.float32(fx["max_length"][b, 0])
            s["mask"] = step_ref._op_mask(s)
    op = ref.operands_of(cache, batch, fx["actions"], 1, start_state=start)
    assert bool(op["feasible"].all()) and op["all_done"]
    r64 = ref.run(op)
    kept = [int(s) for s in fx["steps_kept"]]
    mask = op["mask"][:, kept].numpy()
    assert np.array_equal(mask, fx["step_mask"].astype(bool)), "masks differ from the recorded ones"
    got, want = r64["logp_all"][:, kept].numpy(), fx["step_logprobs"]
    assert np.array_equal(np.isneginf(got), ~mask)
    np.testing.assert_allclose(got[mask], want[mask], rtol=0, atol=2e-4 if env == "cvrptw" else 1e-5)
    np.testing.assert_allclose(r64["logp"].numpy(), fx["logp_steps"], rtol=0, atol=2e-4 if env == "cvrptw" else 1e-5)
    # the selected log-prob is the entry of the full vector (two code paths of the yardstick)
    sel = r64["logp_all"].gather(-1, op["actions"][..., None]).squeeze(-1)
    np.testing.assert_allclose(sel.numpy(), r64["logp"].numpy(), rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def test_case_table_is_the_one_promised():
    every = [(env, "normal", M, S) for env in rc.ENVS for M in ((20, 65) if env == "tsp" else (21, 65)) for S in (1, 4)]
    tsp = [("tsp", k, M, S) for k in rc.KINDS for M in (2, 20, 33, 65, 100, 112, 113, 128, 129) for S in (1, 4, 17)]
    cvrp = [("cvrp", k, M, S) for k in rc.KINDS for M in (21, 65, 112, 113, 129) for S in (1, 4, 17)]
    sdvrp = [("sdvrp", k, M, S) for k in ("normal", "peaked", "tie") for M in (21, 113) for S in (1, 4)]
    assert rc.KINDS == ("normal", "peaked", "policy", "clip0", "temp0.5", "temp2", "saturated", "tie")
    assert set(rc.TABLE) == set(every + tsp + cvrp + sdvrp) and len(rc.TABLE) == len(set(rc.TABLE)) == 366
    assert [rc.clip_temp(dict(kind=k)) for k in rc.KINDS] == [(10.0, 1.0)] * 3 + [(0.0, 1.0), (10.0, 0.5), (10.0, 2.0)] + [(10.0, 1.0)] * 2
    tw = lambda env, M: rc.twins(dict(env=env, kind="tie", M=M))
    assert tw("tsp", 2) == ((0, 1),) and tw("tsp", 20) == ((1, 2), (3, 4), (18, 19))
    assert tw("tsp", 33) == ((1, 2), (3, 4), (31, 32)) and tw("cvrp", 65) == ((1, 2), (3, 4), (31, 32), (63, 64))
    assert tw("cvrp", 129) == ((1, 2), (3, 4), (31, 32), (63, 64), (5, 69), (127, 128)) and tw("sdvrp", 21) == ((1, 2), (3, 4), (19, 20))


@pytest.mark.parametrize("name", [n for n in rc.NAMES if rc.CASES[n]["kind"] == "tie"])
def test_twins_are_bit_identical_in_every_operand(name):
    c, batch, cache, q = rc.operands(name)
    assert rc.twins(c)
    shift = 0 if c["env"] == "tsp" else 1
    for lo, hi in rc.twins(c):
        for k in ("K", "V", "Lp", "Pa", "Pb"):
            assert cache[k] is None or torch.equal(cache[k][:, lo], cache[k][:, hi]), k
        assert torch.equal(q[..., lo], q[..., hi])
        for k, v in batch.items():
            if k in ("locs", "demand", "deterministic_prize", "stochastic_prize", "penalty", "prize"):
                assert np.array_equal(v[:, lo - shift], v[:, hi - shift]), k
            if k in ("time_windows", "durations"):
                assert np.array_equal(v[:, lo], v[:, hi]), k
    assert float(q.min()) > 0


@pytest.mark.parametrize("name", [n for n in rc.NAMES if rc.CASES[n]["kind"] == "saturated"])
def test_saturated_cases_saturate(name):
    assert rc.saturated_share_of_reference(name) >= 0.5


# ---------------------------------------------------------------------------------------------------------------------
# the checks see every mutant, and pass the float32 restatement
# ---------------------------------------------------------------------------------------------------------------------
def stand_in(name, mode, mutant=None):
    """The float32 restatement as a kernel: its decode loop chooses the tour; the log-probs it reports are its own float32
    evaluation of that tour in one batch (with the same mutant).  The loop's step-by-step batches of the same arithmetic round
    differently from the batched run -- up to 1.23 times the bound apart in tsp_peaked_M33_S1, sampling -- which says something
    about batch shapes in a BLAS and nothing about a kernel, so they only select."""
    c, batch, cache, q = rc.operands(name)
    clip, temp = rc.clip_temp(c)
    actions, logps = ref.rollout(cache, batch, c["S"], mode, q, torch.float32, clip, temp, rc.t_max(c), mutant)
    op = ref.operands_of(cache, batch, actions.numpy(), c["S"], 0, clip, temp, mutant)
    if bool(op["feasible"].all()):
        logps = ref.run(op, torch.float32, mutant)["logp"]
    return actions, logps


SEEN_BY = [("glimpse_unmasked", "tsp_normal_M20_S1", "greedy"), ("instance_r_div_S", "cvrp_normal_M21_S4", "greedy"),
           ("rem_of_reset", "sdvrp_peaked_M21_S4", "greedy"), ("state_column_dropped", "cvrp_normal_M21_S1", "greedy"),
           ("state_column_dropped", "cvrptw_normal_M21_S1", "greedy"),
           ("state_column_of_previous_step", "cvrp_normal_M21_S1", "greedy"), ("placeholder_ignored", "tsp_normal_M20_S1", "greedy"),
           ("first_and_current_swapped", "tsp_normal_M20_S1", "greedy"), ("temperature_before_clip", "tsp_temp0.5_M20_S1", "greedy"),
           ("mask_before_clip", "cvrp_normal_M21_S1", "greedy"), ("sampling_minus_noise", "tsp_normal_M20_S1", "sampling"),
           ("tie_to_higher_index", "tsp_tie_M20_S1", "greedy"), ("tie_to_higher_index", "tsp_tie_M20_S1", "sampling"),
           ("tie_to_higher_index", "cvrp_saturated_M21_S1", "greedy")]


@pytest.mark.parametrize("name", rc.NAMES)
def test_float32_restatement_passes_every_check(name):
    for mode in rc.MODES:
        actions, logps = stand_in(name, mode)
        assert rc.check(name, mode, actions, logps)["misses"] == [], mode


@pytest.mark.parametrize("mutant,name,mode", SEEN_BY)
def test_case_table_sees_the_mutant(mutant, name, mode):
    actions, logps = stand_in(name, mode, mutant)
    misses = rc.check(name, mode, actions, logps)["misses"]
    assert misses, (mutant, name)
    if mutant == "tie_to_higher_index":
        assert all(m.startswith(("tie rule", "saturation rule")) for m in misses), misses
    if mutant == "sampling_minus_noise":
        assert all(m.startswith("selection") for m in misses), misses
    assert {m for m, _, _ in SEEN_BY} == set(ref.MUTANTS) - {"rem_of_previous_step"}


@pytest.mark.parametrize("name", ["sdvrp_peaked_M21_S4", "sdvrp_tie_M21_S1"])
def test_stale_remaining_demand_cannot_show_in_a_rollout(name):
    """rem of step t - 1 at step t: the same tours and the same log-probs, bit for bit (why: tests/rollout_ref.py)."""
    for mode in rc.MODES:
        a0, l0 = stand_in(name, mode)
        a1, l1 = stand_in(name, mode, "rem_of_previous_step")
        assert torch.equal(a0, a1) and torch.equal(l0, l1)
