"""GPU: the greedy-rollout baseline on the library's own rollout, the training steps that use it (REINFORCE with
`baseline="rollout"`, the fork's EAM with the attention model's baseline) and one training step recorded from the reference."""
import numpy as np
import pytest
import torch

from _util import golden
from test_gpu_parity import DEV, assert_bits_equal, make_policy, t

import eam_rl4co_amd as ea
from eam_rl4co_amd import train
from eam_rl4co_amd.baselines import as_tensordict

pytestmark = pytest.mark.gpu

ENVS = ["tsp", "cvrp", "op", "pctsp"]
N_EVAL = 64


def _env_policy(env_name, seed=5):
    env = ea.get_env(env_name, generator_params=dict(num_loc=20), seed=seed)
    return env, make_policy("am_" + env_name).train()


def _baseline(env_name, batch_size=64):
    env, pol = _env_policy(env_name)
    rb = ea.RolloutBaseline()
    rb.setup(pol, env, batch_size=batch_size, dataset_size=N_EVAL)
    return env, pol, rb


@pytest.mark.parametrize("env_name", ENVS)
def test_rollout_is_the_policys_greedy_rollout(env_name):
    env, pol, rb = _baseline(env_name)
    assert rb.dataset["locs"].is_cuda and rb.dataset.batch_size[0] == N_EVAL
    assert not rb.policy.training and not any(p.requires_grad for p in rb.policy.parameters())
    r64 = rb.rollout(pol, env, 64)
    assert pol.training and r64.dtype == torch.float32 and r64.shape == (N_EVAL,) and r64.is_cuda
    r7 = rb.rollout(pol, env, 7)
    pol.eval()
    with torch.no_grad():
        want = pol(env.reset(rb.dataset), env, decode_type="greedy")["reward"]
    assert_bits_equal(r64, want, "rollout, one chunk")
    assert_bits_equal(r7, want, "rollout, chunks of 7")
    assert_bits_equal(rb.bl_vals_device, want, "the frozen copy's values")
    assert np.array_equal(rb.bl_vals, want.cpu().numpy().astype(np.float64)) and rb.mean == float(rb.bl_vals.mean())
    # wrap_dataset: "extra" is the frozen copy's rollout, for a dataset on the host and for a TensorDict on the device
    ds = env.dataset([24])
    want = rb.rollout(rb.policy, env, 24, dataset=ds)
    wrapped = rb.wrap_dataset(ds, env, batch_size=7)
    assert not wrapped.extra.is_cuda
    assert_bits_equal(wrapped.extra, want, "extra (dataset)")
    td = as_tensordict(ds, DEV)
    w2 = rb.wrap_dataset(td, env, batch_size=24)
    assert w2["extra"].is_cuda
    assert_bits_equal(w2["extra"], want, "extra (TensorDict)")
    v, loss = rb.eval(env.reset(td), None, env)
    assert loss == 0
    assert_bits_equal(v, want, "eval")


def test_baseline_is_frozen_and_an_accepted_update_takes_the_candidates_values():
    env, pol, rb = _baseline("tsp")
    vals0 = rb.bl_vals_device.clone()
    step = ea.PolicyGradientStep(pol, env, baseline="mean", lr=1e-2)
    td = env.reset(as_tensordict(env.dataset([16]), DEV))
    before = [p.detach().clone() for p in pol.parameters()]
    step(td)
    assert any(not torch.equal(a, b) for a, b in zip(before, pol.parameters()))
    assert_bits_equal(rb.rollout(rb.policy, env, 64), vals0, "frozen baseline after an optimizer step on the policy")
    assert not torch.equal(rb.rollout(pol, env, 64), vals0)
    # an accepted update through epoch_callback: the stored values are made one unit worse on every instance, so the live
    # policy is better with a constant difference (t = -inf, p = 0)
    cand = rb.rollout(pol, env, 64)
    rb.bl_vals = cand.cpu().numpy().astype(np.float64) - 1.0
    rb.mean = float(rb.bl_vals.mean())
    old_ds = rb.dataset
    assert rb.epoch_callback(pol, env=env, batch_size=64, epoch=0, dataset_size=N_EVAL) is True
    assert rb.dataset is not old_ds and pol.training and not rb.policy.training
    for a, b in zip(rb.policy.parameters(), pol.parameters()):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr() and not a.requires_grad
    # the copy's values are the CANDIDATE's greedy rewards on the new dataset, bit for bit (no packed weights of the old copy)
    assert_bits_equal(rb.bl_vals_device, rb.rollout(pol, env, 7), "values after the update")
    assert_bits_equal(rb.rollout(rb.policy, env, 64), rb.bl_vals_device, "the new copy's own rollout")
    # an autograd step directly after the callback works (the live policy's caches were filled under no_grad, not inference mode)
    out = step(td)
    assert torch.isfinite(out["loss"]) and torch.isfinite(out["grad_norm"]) and float(out["grad_norm"]) > 0
    # ... and the copy is still frozen
    assert_bits_equal(rb.rollout(rb.policy, env, 64), rb.bl_vals_device, "the new copy after another step")


def test_policy_gradient_step_with_the_rollout_baseline_over_two_epochs():
    env, pol = _env_policy("tsp")
    step = ea.PolicyGradientStep(pol, env, baseline="rollout")
    wb = step.baseline
    assert isinstance(wb, ea.WarmupBaseline) and isinstance(wb.baseline, ea.RolloutBaseline) and wb.alpha == 0
    step.setup(batch_size=32, dataset_size=N_EVAL)
    for epoch in range(2):
        raw = as_tensordict(env.dataset([32]), DEV)
        data = step.wrap_dataset(raw)
        assert ("extra" in data.keys()) == (epoch == 1)          # the warm-up hands the dataset on unwrapped while alpha == 0
        for i in (0, 16):
            batch = data[i:i + 16]
            extra = batch.get("extra", None)
            out = step(env.reset(batch), extra=extra)
            ll, reward = out["log_likelihood"], out["reward"]
            if epoch == 0:
                assert torch.as_tensor(out["bl_val"]).dim() == 0
            else:
                assert_bits_equal(out["bl_val"], wb.baseline.rollout(wb.baseline.policy, env, 16, dataset=raw[i:i + 16]), "bl_val")
            want = -((reward - out["bl_val"]) * ll).mean() + out["bl_loss"]
            assert torch.equal(out["loss"].detach(), want.detach())
            assert torch.isfinite(out["grad_norm"]) and float(out["grad_norm"]) > 0
            assert all(torch.isfinite(p.grad).all() for p in pol.parameters())
        step.on_epoch_end(epoch)
        assert wb.alpha == 1.0
    assert pol.training


def test_fit_runs_the_epochs():
    env, pol = _env_policy("tsp")
    step = ea.PolicyGradientStep(pol, env, baseline="rollout", baseline_kwargs=dict(n_epochs=2))
    seen = []
    hist = ea.fit(step, env, epochs=3, train_data_size=16, batch_size=8, val_data_size=16, lr_milestones=[1], lr_gamma=0.5,
                  on_step=lambda e, i, out: seen.append((e, i, "bl_val" in out)))
    assert [h["alpha"] for h in hist] == [0.5, 1.0, 1.0] and [h["steps"] for h in hist] == [2, 2, 2]
    assert seen == [(e, i, True) for e in range(3) for i in range(2)]
    assert all(np.isfinite(h["loss"]) and np.isfinite(h["reward"]) and np.isfinite(h["baseline_mean"]) for h in hist)
    assert step.optimizer.param_groups[0]["lr"] == pytest.approx(0.5e-4)


@pytest.mark.parametrize("env_name", ENVS)
def test_eam_am_loss(env_name):
    B = 8
    env, pol, rb = _baseline(env_name)
    torch.manual_seed(4)
    td = env.reset(as_tensordict(env.dataset([B]), DEV))
    extra = rb.eval(td, None, env)[0]
    runner = ea.EA(env, dict(num_generations=3, mutation_rate=0.3, crossover_rate=0.8, selection_rate=0.6, method="am"))
    gen = torch.Generator(device=DEV).manual_seed(9)
    for p in pol.parameters():
        p.grad = None
    out = ea.eam_am_loss(pol, env, td, runner, rb, extra=extra, generator=gen)
    assert out["improved_actions"].shape == out["actions"].shape and out["bl_val"].shape == (2 * B,)
    r_all = torch.cat([out["reward"], out["improved_reward"]])[:, None]
    ll_all = torch.cat([out["log_likelihood"], out["improved_log_likelihood"]])[:, None]
    # the recorded rule (tests/golden/baselines_host.npz, eam_extra_2b): [2B, 1] rewards minus the [2B] values -> [2B, 2B]
    want = -((r_all - torch.cat([extra, extra])) * ll_all).mean()
    assert torch.equal(out["loss"].detach(), want.detach())
    assert out["bl_loss"] == 0
    # improved >= sampled.  OP: a sampled tour that starts at the depot is empty, and what the crossover rebuilds from it is no
    # episode of the env (test_eam_single_start_improvement) -- such a row keeps its sampled tour
    assert (out["improved_reward"] >= out["reward"] - 1e-5).all()
    if env_name == "op":
        empty = out["actions"][:, 0] == 0
        assert torch.equal(out["improved_actions"][empty], out["actions"][empty])
    env.check_solution_validity(td, out["improved_actions"])
    assert torch.isfinite(out["improved_log_likelihood"]).all() and torch.isfinite(out["log_likelihood"]).all()
    assert torch.isfinite(out["loss"])
    out["loss"].backward()
    g = pol.encoder.init_embedding.init_embed.weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0
    # given draws (the EA's random inputs as tensors): the improved tours are the EA's on the sampled tours under these draws
    T = out["actions"].shape[1]
    if env_name == "tsp":
        draws = ea.EADraws.sample(3, B, 50, T, 0.6, DEV, torch.Generator(device=DEV).manual_seed(3))
    elif env_name == "cvrp":
        draws = ea.EACvrpDraws.sample(3, B, 50, 0.6, DEV, torch.Generator(device=DEV).manual_seed(3))
    else:
        draws = ea.EAPrizeDraws.sample(3, B, 50, 0.6, DEV, torch.Generator(device=DEV).manual_seed(3))
    out = ea.eam_am_loss(pol, env, td, runner, rb, extra=extra, draws=draws, return_entropy=False)
    want, _ = ea.evolution_worker(out["actions"], td, runner, env, draws=draws)
    if env_name == "op":
        empty = out["actions"][:, 0] == 0
        want = torch.where(empty[:, None], out["actions"], want)
    assert torch.equal(out["improved_actions"], want)
    if env_name == "tsp":       # evaluated on the fly: the frozen copy's greedy rewards of the doubled batch, row by row
        out = ea.eam_am_loss(pol, env, td, runner, rb, generator=gen, return_entropy=False)
        assert out["bl_val"].shape == (2 * B, 1)
        assert_bits_equal(out["bl_val"][:, 0], torch.cat([extra, extra]), "bl_val on the fly")
        out = ea.eam_am_loss(pol, env, td, runner, rb, extra=extra, improve=False)
        assert out["bl_val"].shape == (B, 1) and "improved_reward" not in out
        assert torch.equal(out["loss"].detach(), -((out["reward"] - extra) * out["log_likelihood"]).mean().detach())


def test_reference_training_step_with_the_rollout_baseline():
    """AM TSP-20, one REINFORCE step with the rollout baseline recorded from the reference (make_golden_baselines.py): the
    baseline's values, the sampled step and every gradient, at the tolerance of tests/test_gpu_train.py's training fixtures."""
    fx = golden("train_am_tsp20_rollout")
    env = ea.get_env("tsp", generator_params=dict(num_loc=20))
    pol = make_policy("am_tsp").train()
    rb = ea.RolloutBaseline()
    eval_ds = ea.TensorDict({"locs": torch.from_numpy(fx["eval_locs"])}, batch_size=[fx["eval_locs"].shape[0]])
    rb.setup(pol, env, batch_size=5, dataset=eval_ds)
    np.testing.assert_allclose(rb.bl_vals, fx["bl_vals"].astype(np.float64), rtol=1e-6)
    np.testing.assert_allclose(rb.mean, float(fx["bl_mean"]), rtol=1e-6)
    batch = rb.wrap_dataset(ea.TensorDict({"locs": t(fx["locs"])}, batch_size=[fx["locs"].shape[0]]), env, batch_size=3)
    np.testing.assert_allclose(batch["extra"].cpu().numpy(), fx["extra"], rtol=1e-6)
    td = env.reset(batch)
    out = train.reinforce_loss(pol, env, td, baseline=rb, extra=batch["extra"], select_best=False, noise=t(fx["noise"]))
    assert_bits_equal(out["actions"], fx["actions"], "actions")
    np.testing.assert_allclose(out["reward"].cpu().numpy(), fx["reward"], rtol=1e-6)
    np.testing.assert_allclose(out["log_likelihood"].detach().cpu().numpy(), fx["logp_steps"].sum(1), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(out["bl_val"].cpu().numpy(), fx["bl_val"], rtol=1e-6)
    np.testing.assert_allclose(float(out["loss"].detach()), float(fx["loss"]), rtol=2e-5)
    out["loss"].backward()
    params = dict(pol.named_parameters())
    total_ref = float(np.sqrt((fx["grad_norms"] ** 2).sum()))
    for k, ref_norm in zip(fx["grad_names"], fx["grad_norms"]):
        g = params[str(k)].grad
        got = 0.0 if g is None else float(g.double().norm())
        assert abs(got - ref_norm) <= 1e-4 * max(ref_norm, 1e-3 * total_ref) + 1e-7, (str(k), got, ref_norm)
        if "grad__" + str(k) in fx and g is not None:
            ref = fx["grad__" + str(k)]
            np.testing.assert_allclose(g.cpu().numpy(), ref, rtol=0, atol=1e-4 * max(float(np.abs(ref).max()), 1e-3 * total_ref),
                                       err_msg=str(k))
