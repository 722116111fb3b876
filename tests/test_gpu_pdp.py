"""GPU: the pickup-and-delivery (PDP) path -- step / validity / init-embedding kernels and the three decode kernels through
`policy(td, env, ...)` -- against tests/pdp_ref.py, BIT FOR BIT (integers, masks and every float: both sides evaluate the same
defined order), and hence against the reference's recorded tours (tests/test_host_pdp.py pins pdp_ref to those).

Invalid tours are inputs of the validity kernel only; no rollout is ever fed one.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pdp_ref
from _util import golden
from test_gpu_parity import DEV, assert_bits_equal, t

pytestmark = pytest.mark.gpu

POMO = dict(num_encoder_layers=6, normalization="instance", use_graph_context=False)


def make_policy(cfg="am_pdp", **kw):
    import eam_rl4co_amd as ea

    if cfg.startswith("pomo"):
        kw = dict(POMO, **kw)
    pol = ea.AttentionModelPolicy(env_name="pdp", **kw).eval()
    sd = pol.state_dict()
    for k, v in pdp_ref.weights(cfg).items():
        sd[k].copy_(torch.from_numpy(v))
    return pol.to(DEV)


def make_td(locs, force_start_at_depot=False):
    """Post-reset TensorDict on the GPU from recorded locs [B, N + 1, 2] (depot first)."""
    import eam_rl4co_amd as ea

    env = ea.PDPEnv(generator_params=dict(num_loc=locs.shape[1] - 1), force_start_at_depot=force_start_at_depot)
    td = ea.TensorDict({"locs": torch.from_numpy(np.ascontiguousarray(locs[:, 1:])),
                        "depot": torch.from_numpy(np.ascontiguousarray(locs[:, 0]))}, batch_size=[locs.shape[0]])
    return env, env.reset(td).to(DEV)


def call_kwargs(fx):
    kw = dict(return_sum_log_likelihood=False)
    decode_type = str(fx["decode_type"])
    if decode_type == "evaluate":
        kw["actions"] = t(fx["actions"])
        decode_type = "sampling"
    kw["decode_type"] = decode_type
    if int(fx["num_starts"]) > 1:
        kw["num_starts"] = int(fx["num_starts"])
    if "noise" in fx:
        kw["noise"] = t(fx["noise"])
    for k in ("top_k", "top_p"):
        if "decode_kw_" + k in fx:
            kw[k] = fx["decode_kw_" + k].item()
    return kw


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_step_mask_kernel_on_the_recorded_trace():
    from eam_rl4co_amd import ops

    fx = golden("env_pdp20_random")
    B, N = fx["gen_locs"].shape[:2]
    ref = pdp_ref.Env(B, N)
    visited, to_deliver = t(~ref.available), t(ref.to_deliver)
    cur = torch.zeros(B, dtype=torch.int64, device=DEV)
    done = torch.zeros(B, dtype=torch.bool, device=DEV)
    mask = torch.zeros(B, N + 1, dtype=torch.bool, device=DEV)
    ops.pdp_step_mask_(visited, to_deliver, None, None, mask)              # mask only: the reset mask
    assert_bits_equal(mask, ref.action_mask, "reset mask")
    for s in range(fx["step_action"].shape[1]):
        a = fx["step_action"][:, s]
        ref.step(a)
        ops.pdp_step_mask_(visited, to_deliver, cur, t(a), mask, done)
        for got, k in ((mask, "action_mask"), (~visited, "available"), (to_deliver, "to_deliver"), (done, "done")):
            assert_bits_equal(got, getattr(ref, k), f"{k} after step {s}")
            assert_bits_equal(got, fx["step_" + k][:, s], f"{k} after step {s} (reference)")
        assert_bits_equal(cur, ref.current_node, f"current_node after step {s}")
    assert bool(done.all())


def test_validity_kernel_verdict_by_verdict():
    from eam_rl4co_amd import ops

    fx = golden("pdp_validity_cases")
    N, acts, want = int(fx["num_loc"]), fx["actions"], fx["verdict"]
    assert np.array_equal(pdp_ref.check_solution(acts, N), want)
    dev = t(acts)
    for i in range(acts.shape[0]):
        bad = ops.check_solution("pdp", dev[i:i + 1].contiguous(), num_loc=N).tolist()
        got = pdp_ref.NOT_ALL_NODES if bad[0] else (pdp_ref.DELIVERY_FIRST if bad[1] else pdp_ref.VALID)
        assert got == want[i] and sum(bad) <= 1, f"row {i} {acts[i].tolist()}: counters {bad}, the reference's verdict {want[i]}"
    counts = [int((want == pdp_ref.NOT_ALL_NODES).sum()), int((want == pdp_ref.DELIVERY_FIRST).sum())]
    assert ops.check_solution("pdp", dev, num_loc=N).tolist() == counts            # all rows at once: several blocks
    # the same verdicts through the rollout epilogue, with the reward of the single-purpose kernel
    locs = t(np.random.default_rng(0).random((1, N + 1, 2), dtype=np.float32))
    inr = (acts >= 0).all(1) & (acts <= N).all(1)
    bad = torch.zeros(2, dtype=torch.int32, device=DEV)
    reward, _ = ops.rollout_finish("pdp", locs, dev, bad=bad)
    assert bad.tolist() == counts
    assert_bits_equal(reward[t(inr)], ops.tour_length_reward(locs, dev[t(inr)].contiguous(), with_depot=True), "reward")
    # force_start_at_depot tours hold the depot themselves: first (or, as the reference accepts, last) position
    valid = acts[want == pdp_ref.VALID]
    lead = np.concatenate([np.zeros((valid.shape[0], 1), np.int64), valid], 1)
    trail = np.concatenate([valid, np.zeros((valid.shape[0], 1), np.int64)], 1)
    inside = lead.copy()
    inside[:, [0, 3]] = inside[:, [3, 0]]
    for rows, verdict in ((lead, pdp_ref.VALID), (trail, pdp_ref.VALID), (inside, pdp_ref.NOT_ALL_NODES)):
        assert (pdp_ref.check_solution(rows, N, force_start_at_depot=True) == verdict).all()
        assert ops.check_solution("pdp", t(rows), num_loc=N).tolist() == [rows.shape[0] * (verdict != pdp_ref.VALID), 0]


@pytest.mark.parametrize("name", ["pdp4_greedy", "pdp20_greedy"])
def test_init_embedding_bit_exact(name):
    from eam_rl4co_amd import ops

    fx = golden(name)
    locs = fx["locs"]
    assert locs.shape[1] in (5, 21)
    for cfg in ("am_pdp", "pomo_pdp"):
        pol = make_policy(cfg)
        sd = pdp_ref.weights(cfg)
        want = pdp_ref.init_embedding(sd, locs)
        _, td = make_td(locs)
        got = pol.encoder.init_embedding(td)
        assert_bits_equal(got, want, f"{cfg} init embedding")
        ie, half, L = pol.encoder.init_embedding, (locs.shape[1] - 1) // 2, td["locs"]
        three = torch.cat((ops.linear(L[:, :1].contiguous(), ie.init_embed_depot.weight, ie.init_embed_depot.bias),
                           ops.linear(torch.cat((L[:, 1:half + 1], L[:, half + 1:]), -1).contiguous(), ie.init_embed_pick.weight,
                                      ie.init_embed_pick.bias),
                           ops.linear(L[:, half + 1:].contiguous(), ie.init_embed_delivery.weight, ie.init_embed_delivery.bias)), 1)
        assert torch.equal(got, three), "one launch != the three linears"


# ---------------------------------------------------------------------------------------------------------------------
# policy level: whole-rollout kernels and the step-wise path against pdp_ref, fixture by fixture
# ---------------------------------------------------------------------------------------------------------------------
KERNEL = {"pdp4_greedy": "resident", "pdp20_greedy": "resident", "pdp20_sampling": "resident", "pdp20_evaluate": "resident",
          "pdp20_sampling_topk5": "resident", "pdp20_sampling_topp09": "resident", "pomo_pdp20_multistart_greedy": "resident",
          "pdp110_greedy": "resident", "pdp126_greedy": "resident", "pdp128_greedy": "stream",
          "pdp20_greedy_depot_start": "resident"}


def expected_kernel(B, M, R, t_max, top_k=0, top_p=0.0):
    from eam_rl4co_amd import _lib, ops

    cs = _lib.Cache()
    cs.B, cs.M, cs.E, cs.H, cs.ld = B, M, 128, 8, (5 * 128 if M <= 128 else 128)
    return ops.rollout_kernel("pdp", cs, R, t_max, top_k, top_p)


@pytest.mark.parametrize("name", pdp_ref.ROLLOUT_FIXTURES)
def test_policy_rollout_bit_exact(name):
    fx, ref = pdp_ref.reference(name)
    force = bool(fx["force_start_at_depot"])
    pol = make_policy(pdp_ref.cfg_for(fx))
    env, td = make_td(fx["locs"], force)
    kw = call_kwargs(fx)
    B, M = fx["locs"].shape[:2]
    S = max(int(fx["num_starts"]), 1)
    t_max = M - 1 + int(force) - (1 if S > 1 else 0)
    assert expected_kernel(B, M, B * S, t_max, kw.get("top_k", 0), kw.get("top_p", 0.0)) == KERNEL[name]
    assert set(KERNEL) == set(pdp_ref.ROLLOUT_FIXTURES)
    outs = []
    for stepwise in (False, True):
        out = pol(td, env, phase="test", store_all_logp=stepwise, **kw)
        assert_bits_equal(out["actions"], ref["actions"], f"tours (stepwise={stepwise})")
        assert_bits_equal(out["actions"], fx["actions"], "tours against the reference")
        assert_bits_equal(out["log_likelihood"], ref["logp_steps"], f"per-step log-probs (stepwise={stepwise})")
        assert_bits_equal(out["reward"], ref["reward"], f"reward (stepwise={stepwise})")
        last = pol._last_td
        assert_bits_equal(last["available"], ref["final_available"], "final available")
        assert_bits_equal(last["to_deliver"], ref["final_to_deliver"], "final to_deliver")
        assert not bool(last["action_mask"].any()) and bool(last["done"].all())
        assert int(last["i"].reshape(-1)[0]) == ref["actions"].shape[1]
        outs.append(out)
    np.testing.assert_allclose(outs[0]["reward"].cpu().numpy(), fx["reward"], rtol=1e-6)
    # the same call on the streaming kernel (the switch the other envs' tests use)
    if KERNEL[name] != "stream":
        from eam_rl4co_amd import _lib

        lib = _lib.load()
        lib.eamrl_debug_set(1, 1)
        try:
            assert expected_kernel(B, M, B * S, t_max, kw.get("top_k", 0), kw.get("top_p", 0.0)) == "stream"
            out = pol(td, env, phase="test", **kw)
        finally:
            lib.eamrl_debug_set(1, 0)
        assert_bits_equal(out["actions"], ref["actions"], "tours (streaming)")
        assert_bits_equal(out["log_likelihood"], ref["logp_steps"], "per-step log-probs (streaming)")


def test_filtering_variant_limit_and_multistart_dispatch():
    """Filtered calls stay resident up to 112 nodes and stream above; PDP multistart batches never go to the start-sharing
    MFMA kernel (which has no PDP case) -- the dispatcher hands them to the resident kernel."""
    assert expected_kernel(2, 111, 2, 110, top_k=5) == "resident"
    assert expected_kernel(2, 113, 2, 112, top_k=5) == "stream"
    assert expected_kernel(2, 113, 2, 112) == "resident"
    assert expected_kernel(4, 21, 40, 19) == "resident"
    assert expected_kernel(4, 129, 40, 127) == "stream"


def test_evaluate_reproduces_the_greedy_log_likelihood():
    fx, ref = pdp_ref.reference("pdp20_greedy")
    pol = make_policy()
    env, td = make_td(fx["locs"])
    g = pol(td, env, phase="test", decode_type="greedy", return_sum_log_likelihood=False)
    e = pol(td, env, phase="test", actions=g["actions"], return_sum_log_likelihood=False)
    assert_bits_equal(e["log_likelihood"], g["log_likelihood"], "evaluate vs greedy")
    assert_bits_equal(e["reward"], g["reward"], "reward")
    s = pol(td, env, phase="test", actions=g["actions"])
    from oracle import oracle as orc
    assert_bits_equal(s["log_likelihood"], orc.sum_logp(ref["logp_steps"]), "summed log-likelihood")


def test_multistart_per_start_tours_and_select_best():
    fx, ref = pdp_ref.reference("pomo_pdp20_multistart_greedy")
    pol = make_policy("pomo_pdp")
    env, td = make_td(fx["locs"])
    B, S = fx["locs"].shape[0], int(fx["num_starts"])
    assert env.get_num_starts(td) == S
    out = pol(td, env, phase="test", decode_type="multistart_greedy")          # num_starts from the env
    assert_bits_equal(out["actions"], fx["actions"], "per-start tours")
    assert_bits_equal(out["actions"][:, 0], pdp_ref.select_start_nodes(B, 20, S), "start nodes")
    best = pol(td, env, phase="test", decode_type="multistart_greedy", num_starts=S, select_best=True)
    idx = ref["reward"].reshape(S, B).argmax(0) * B + np.arange(B)
    assert_bits_equal(best["actions"], ref["actions"][idx], "best tours")
    assert_bits_equal(best["reward"], ref["reward"][idx], "best rewards")


def test_seeded_sampling_equals_noise_fed_rollout():
    from eam_rl4co_amd import ops
    from eam_rl4co_amd.policy import state_from_td

    fx = golden("pdp20_sampling")
    pol = make_policy()
    _, td = make_td(fx["locs"])
    with torch.no_grad():
        hidden, _ = pol.encoder(td)
        cache = pol.decoder._precompute_cache(hidden)
    B, M = fx["locs"].shape[:2]
    a1, l1, i1 = ops.rollout(state_from_td("pdp", td), cache, "sampling", seed=20240607, t_max=M - 1)
    noise = ops.exp1_noise(20240607, B, M - 1, M, DEV)
    a2, l2, i2 = ops.rollout(state_from_td("pdp", td), cache, "sampling", noise=noise, t_max=M - 1)
    assert i1.tolist() == [M - 1, 0] and i2.tolist() == [M - 1, 0]
    assert_bits_equal(a1, a2, "tours")
    assert_bits_equal(l1, l2, "log-probs")
    assert (pdp_ref.check_solution(a1.cpu().numpy(), M - 1) == pdp_ref.VALID).all()


@pytest.mark.parametrize("mode", ["greedy", "sampling"])
def test_graphed_rollout_equals_eager(mode):
    import eam_rl4co_amd as ea

    pol = make_policy()
    env = ea.get_env("pdp", generator_params=dict(num_loc=20), seed=3)
    tds = [env.reset(batch_size=[16]).to(DEV) for _ in range(3)]
    kw = {}
    if mode == "sampling":
        kw["noise"] = torch.empty(16, 20, 21, device=DEV).exponential_(1)
    g = ea.GraphedRollout(pol, env, tds[0], decode_type=mode, **kw)
    for td in tds + [tds[0]]:
        a = g(td)
        b = pol(td.clone(), env, phase="test", decode_type=mode, **kw)
        assert_bits_equal(a["actions"], b["actions"], "actions")
        assert_bits_equal(a["reward"], b["reward"], "reward")
        assert_bits_equal(a["log_likelihood"], b["log_likelihood"], "ll")


@pytest.mark.parametrize("method", ["greedy", "sampling", "multistart_greedy", "augment_dihedral_8", "augment",
                                    "multistart_greedy_augment_dihedral_8", "multistart_greedy_augment"])
def test_evaluators_return_valid_tours(method):
    import eam_rl4co_amd as ea
    from eam_rl4co_amd.eval import evaluate_policy

    env = ea.get_env("pdp", generator_params=dict(num_loc=20), seed=13)
    pol = make_policy()
    ds = env.dataset(batch_size=[16], phase="test")
    res = evaluate_policy(env, pol, ds, method=method, samples=4)
    assert res["rewards"].shape == (16,) and res["actions"].shape == (16, 20)
    assert torch.isfinite(res["rewards"]).all()
    assert (pdp_ref.check_solution(res["actions"].numpy(), 20) == pdp_ref.VALID).all()


def test_beam_search_runs_through_the_generic_code():
    fx = golden("pdp20_greedy")
    pol = make_policy()
    env, td = make_td(fx["locs"])
    out = pol(td, env, phase="test", decode_type="beam_search", beam_width=4)
    assert (pdp_ref.check_solution(out["actions"].cpu().numpy(), 20) == pdp_ref.VALID).all()
    greedy = pol(td, env, phase="test", decode_type="greedy")
    assert out["reward"].shape == greedy["reward"].shape and torch.isfinite(out["reward"]).all()


def test_reevaluation_and_one_reinforce_step():
    """The PyTorch re-evaluation path (`_pdp_states`): its per-step log-probs against the rollout's and the reference's within the
    tolerance of test_gpu_next.py::test_reevaluation_matches_native_logp_and_reference (abs 1e-4), and one REINFORCE step with
    finite, non-zero gradients on the three init-embedding layers and on project_context."""
    from eam_rl4co_amd.train import evaluate_log_likelihood, native_reeval_supported, reinforce_loss

    fx = golden("pdp20_sampling")
    pol = make_policy()
    env, td = make_td(fx["locs"])
    assert not native_reeval_supported(pol, 21)
    native = pol(td, env, phase="test", decode_type="sampling", noise=t(fx["noise"]), return_sum_log_likelihood=False)
    logp = evaluate_log_likelihood(pol, td, env, native["actions"])
    assert logp.requires_grad
    np.testing.assert_allclose(logp.detach().cpu().numpy(), native["log_likelihood"].cpu().numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(logp.detach().cpu().numpy(), fx["logp_steps"], rtol=0, atol=1e-4)
    pol.train()
    torch.manual_seed(0)
    out = reinforce_loss(pol, env, td.clone(), baseline="mean")
    assert out["actions"].shape == (8, 20) and out["log_likelihood"].requires_grad
    pol.zero_grad()
    out["loss"].backward()
    ie = pol.encoder.init_embedding
    for name, p in (("depot", ie.init_embed_depot.weight), ("pick", ie.init_embed_pick.weight),
                    ("delivery", ie.init_embed_delivery.weight), ("depot bias", ie.init_embed_depot.bias),
                    ("project_context", pol.decoder.context_embedding.project_context.weight)):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, name


def test_bf16_mixed_greedy_returns_valid_tours():
    fx = golden("pdp20_greedy")
    pol = make_policy(precision="bf16-mixed")
    env, td = make_td(fx["locs"])
    out = pol(td, env, phase="test", decode_type="greedy")
    assert (pdp_ref.check_solution(out["actions"].cpu().numpy(), 20) == pdp_ref.VALID).all()
    assert torch.isfinite(out["reward"]).all() and torch.isfinite(out["log_likelihood"]).all()
    np.testing.assert_allclose(out["reward"].cpu().numpy(), env.get_reward(td, out["actions"]).cpu().numpy(), rtol=0, atol=0)


def test_env_step_api_and_force_start():
    """env.step on the GPU follows the recorded trace; with force_start_at_depot the first feasible action is the depot."""
    import eam_rl4co_amd as ea

    fx = golden("env_pdp20_random")
    locs = np.concatenate([fx["gen_depot"][:, None], fx["gen_locs"]], 1)
    env, td = make_td(locs)
    assert_bits_equal(env.get_action_mask(td), fx["reset_action_mask"], "get_action_mask")
    for s in range(fx["step_action"].shape[1]):
        td.set("action", t(fx["step_action"][:, s]))
        td = env.step(td)["next"]
        for k in ("action_mask", "available", "to_deliver", "done", "current_node"):
            assert_bits_equal(td[k], fx["step_" + k][:, s], f"{k} after step {s}")
    assert_bits_equal(td["i"], np.full((locs.shape[0], 1), 20), "i")
    np.testing.assert_allclose(env.get_reward(td, t(fx["step_action"])).cpu().numpy(), fx["reward"], rtol=1e-6)
    with pytest.raises(AssertionError, match="Deliverying without pick-up"):
        env.check_solution_validity(td, t(np.roll(np.arange(1, 21), 10)[None].repeat(locs.shape[0], 0)))
    env2, td2 = make_td(locs, force_start_at_depot=True)
    assert td2["action_mask"][:, 0].all() and not td2["action_mask"][:, 1:].any()
    td2.set("action", torch.zeros(locs.shape[0], dtype=torch.int64, device=DEV))
    td2 = env2.step(td2)["next"]
    assert_bits_equal(td2["action_mask"], fx["reset_action_mask"], "mask after the forced depot step")
