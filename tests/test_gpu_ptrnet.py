"""GPU: the Pointer Network policy on its two one-launch kernels (csrc/ptrnet.hip).

Fixture parity (tests/golden/make_golden_ptrnet.py ran the reference): identical tours, reward at rtol 1e-6, and per-step
log-probs within max(4 e32, 1e-6) of the reference's float64 run, e32 being the error of the float32 run of the restatement
tests/ptrnet_ref.py on that fixture -- the criterion of tests/test_gpu_reeval.py: the kernel may be as wrong as plain float32
arithmetic is, four times over, and no more.  The same bound holds at the kernel-boundary shapes against the restatement in
float64.  Every figure is printed before it is asserted.
"""
import functools

import numpy as np
import pytest
import torch

import ptrnet_ref
from _util import golden
from test_host_ptrnet import FIXTURES, SHAPES

pytestmark = pytest.mark.gpu

DEV = "cuda"
MIN_GAP = 1e-4
ENC_TILE, DEC_TILE = 16, 4            # instances per workgroup of k_ptrnet_encode / k_ptrnet_rollout


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def weights(dtype):
    return {k: v.to(DEV) for k, v in ptrnet_ref.closed_form_weights(SHAPES, dtype).items()}


@functools.lru_cache(maxsize=None)
def policy():
    import eam_rl4co_amd as ea

    pol = ea.PointerNetworkPolicy().eval()
    pol.load_state_dict(ptrnet_ref.closed_form_weights(SHAPES))
    return pol.to(DEV)


def make_td(locs):
    import eam_rl4co_amd as ea

    env = ea.TSPEnv(generator_params=dict(num_loc=locs.shape[1]))
    td = ea.TensorDict({"locs": torch.as_tensor(locs).float().cpu()}, batch_size=[locs.shape[0]])
    return env, env.reset(td).to(DEV)


def call_kw(fx):
    mode = str(fx["decode_type"])
    if mode == "sampling":
        return dict(decode_type="sampling", noise=t(fx["noise"]))
    if mode == "evaluate":
        return dict(actions=t(fx["actions"]))
    return dict(decode_type="greedy")


@functools.lru_cache(maxsize=None)
def rolled(name):
    fx = golden(name)
    env, td = make_td(fx["locs"])
    with torch.no_grad():
        out = policy()(td, env, phase="test", return_sum_log_likelihood=False, **call_kw(fx))
    return fx, env, td, out


def e32_of(locs, tours):
    """max |float32 restatement - float64 restatement| of the chosen-node log-probs on given tours: (e32, logp64)."""
    lp64 = ptrnet_ref.rollout(weights(torch.float64), locs, "evaluate", given=tours)[1]
    lp32 = ptrnet_ref.rollout(weights(torch.float32), locs, "evaluate", given=tours)[1]
    return float((lp32.double() - lp64).abs().max()), lp64


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_parity(name):
    fx, env, td, out = rolled(name)
    assert np.array_equal(out["actions"].cpu().numpy(), fx["actions"]), "tours"
    np.testing.assert_allclose(out["reward"].cpu().numpy(), fx["reward"], rtol=1e-6)
    e32, _ = e32_of(t(fx["locs"]), t(fx["actions"]))
    err = float(np.abs(out["log_likelihood"].double().cpu().numpy() - fx["logp64"]).max())
    bound = max(4 * e32, 1e-6)
    print(f"PTRNET {name}: kernel error {err:.3e}, float32 restatement error {e32:.3e}, ratio {err / max(e32, 2.5e-7):.2f} "
          f"(bound {bound:.3e})")
    assert err <= bound


def test_evaluate_reproduces_the_rollout_bit_for_bit():
    fx, env, td, out = rolled("ptrnet20_sampling")
    with torch.no_grad():
        again = policy()(td, env, phase="test", actions=out["actions"], return_sum_log_likelihood=False)
        tours = policy()(td, env, phase="test", eval_tours=out["actions"])
    assert torch.equal(again["actions"], out["actions"])
    assert torch.equal(again["log_likelihood"], out["log_likelihood"])
    assert torch.equal(tours["log_likelihood"], out["log_likelihood"].sum(1))
    assert torch.equal(again["reward"], out["reward"])


@pytest.mark.parametrize("n, b", [(20, 5), (113, 2)])
def test_seeded_sampling_equals_the_call_with_the_noise_tensor(n, b):
    import eam_rl4co_amd as ea

    torch.manual_seed(n)
    env, td = make_td(torch.rand(b, n, 2))
    seed = 0x1234_5678_9ABC_DEF0 + n
    with torch.no_grad():
        a = policy()(td, env, phase="test", decode_type="sampling", seed=seed, return_sum_log_likelihood=False)
        noise = ea.ops.exp1_noise(seed, b, n, n, device=DEV)
        c = policy()(td, env, phase="test", decode_type="sampling", noise=noise, return_sum_log_likelihood=False)
    assert torch.equal(a["actions"], c["actions"]) and torch.equal(a["log_likelihood"], c["log_likelihood"])
    assert sorted(a["actions"][0].tolist()) == list(range(n))


# every N with full and tail tiles of both kernels (33 = 2 * 16 + 1 = 8 * 4 + 1); every B around both tiles at an N on each
# side of the 64-node lane round
SHAPE_CASES = ([(n, 33) for n in (2, 3, 16, 17, 64, 65, 127, 128)]
               + [(n, b) for n in (17, 65) for b in (1, DEC_TILE - 1, DEC_TILE, DEC_TILE + 1, ENC_TILE - 1, ENC_TILE, ENC_TILE + 1)])


def shape_case(n, b):
    """(locs [b, n, 2] on the CPU, seed): the data and the sampling seed of a kernel-boundary case."""
    g = torch.Generator().manual_seed(7000 + 131 * n + b)
    return torch.rand(b, n, 2, generator=g), 9000 + 131 * n + b


@pytest.mark.parametrize("n, b", SHAPE_CASES)
def test_kernel_boundary_shapes_against_the_float64_restatement(n, b):
    import eam_rl4co_amd as ea

    locs, seed = shape_case(n, b)
    env, td = make_td(locs)
    before = {k: v.clone() for k, v in policy().state_dict().items()}
    with torch.no_grad():
        out = policy()(td, env, phase="test", decode_type="sampling", seed=seed, return_sum_log_likelihood=False)
    noise = ea.ops.exp1_noise(seed, b, n, n, device=DEV)
    ref_a, _, gap = ptrnet_ref.rollout(weights(torch.float64), locs.to(DEV), "sampling", noise=noise)
    keep = gap >= MIN_GAP
    frac = float(keep.double().mean())
    print(f"PTRNET shape N={n} B={b}: {int(keep.sum())} of {b} rows have a decision margin >= {MIN_GAP}")
    assert frac >= 0.9
    assert torch.equal(out["actions"][keep], ref_a[keep]), "tours"
    for row in out["actions"].tolist():
        assert sorted(row) == list(range(n))
    e32, lp64 = e32_of(locs.to(DEV), out["actions"])
    err = float((out["log_likelihood"].double() - lp64).abs().max())
    bound = max(4 * e32, 1e-6)
    print(f"PTRNET shape N={n} B={b}: kernel error {err:.3e}, float32 restatement error {e32:.3e} (bound {bound:.3e})")
    assert err <= bound
    for k, v in policy().state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed during a rollout"


def test_train_step_matches_the_reference_gradients():
    import eam_rl4co_amd as ea

    fx = golden("train_ptrnet_tsp20")
    pol = ea.PointerNetworkPolicy()
    pol.load_state_dict(ptrnet_ref.closed_form_weights(SHAPES))
    pol = pol.to(DEV).train()
    env, td = make_td(fx["locs"])
    out = pol(td, env, phase="train", decode_type="sampling", noise=t(fx["noise"]))
    assert np.array_equal(out["actions"].cpu().numpy(), fx["actions"]), "actions"
    np.testing.assert_allclose(out["reward"].cpu().numpy(), fx["reward"], rtol=1e-6)
    ll, reward = out["log_likelihood"], out["reward"]
    assert ll.requires_grad and ll.grad_fn is not None and ll.shape == (fx["locs"].shape[0],)
    loss = -((reward - reward.mean()) * ll).mean()
    print(f"PTRNET train_ptrnet_tsp20: loss {float(loss.detach()):.8f} reference {float(fx['loss']):.8f}")
    np.testing.assert_allclose(float(loss.detach()), float(fx["loss"]), rtol=2e-5)
    loss.backward()
    params = dict(pol.named_parameters())
    total_ref = float(np.sqrt((fx["grad_norms"] ** 2).sum()))
    worst = 0.0
    for key, ref_norm in zip(fx["grad_names"], fx["grad_norms"]):
        g = params[str(key)].grad
        got = 0.0 if g is None else float(g.double().norm())
        worst = max(worst, abs(got - ref_norm) / max(ref_norm, 1e-3 * total_ref))
    print(f"PTRNET train_ptrnet_tsp20: largest relative gradient-norm difference {worst:.3e}")
    assert params["encoder.init_hx"].grad is None and params["encoder.init_cx"].grad is None
    for key, ref_norm, present in zip(fx["grad_names"], fx["grad_norms"], fx["grad_present"]):
        g = params[str(key)].grad
        assert (g is not None) == bool(present), str(key)
        got = 0.0 if g is None else float(g.double().norm())
        assert abs(got - ref_norm) <= 1e-4 * max(ref_norm, 1e-3 * total_ref), (str(key), got, ref_norm)
        if "grad__" + str(key) in fx:
            ref = fx["grad__" + str(key)]
            np.testing.assert_allclose(g.cpu().numpy(), ref, rtol=0, atol=1e-4 * max(float(np.abs(ref).max()), 1e-3 * total_ref),
                                       err_msg=str(key))


def test_reinforce_loss_and_an_adam_step_move_the_pointer():
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import train

    fx = golden("train_ptrnet_tsp20")
    pol = ea.PointerNetworkPolicy()
    pol.load_state_dict(ptrnet_ref.closed_form_weights(SHAPES))
    pol = pol.to(DEV)
    env, td = make_td(fx["locs"])
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
    v0 = pol.decoder.pointer.v.detach().clone()
    for baseline in ("mean", "no"):
        opt.zero_grad()
        res = train.reinforce_loss(pol, env, td, baseline=baseline, noise=t(fx["noise"]))
        assert np.array_equal(res["actions"].cpu().numpy(), fx["actions"])
        if baseline == "mean":
            np.testing.assert_allclose(float(res["loss"].detach()), float(fx["loss"]), rtol=2e-5)
        res["loss"].backward()
    opt.step()
    assert not torch.equal(pol.decoder.pointer.v.detach(), v0)


def test_policy_gradient_step_runs_unchanged():
    import eam_rl4co_amd as ea

    fx = golden("train_ptrnet_tsp20")
    pol = ea.PointerNetworkPolicy().to(DEV)
    env, td = make_td(fx["locs"])
    step = ea.PolicyGradientStep(pol, env, baseline="mean", lr=1e-3)
    v0 = pol.decoder.pointer.v.detach().clone()
    res = step(td)
    assert torch.isfinite(torch.as_tensor(res["loss"])).all()
    assert not torch.equal(pol.decoder.pointer.v.detach(), v0)


def test_checkpoint_round_trip(tmp_path):
    import eam_rl4co_amd as ea

    fx, env, td, out = rolled("ptrnet20_greedy")
    sd = {"policy." + k: v.cpu() for k, v in policy().state_dict().items()}
    sd["baseline.baseline.policy.embedding"] = torch.zeros(2, 128)
    path = tmp_path / "ptrnet.ckpt"
    torch.save({"state_dict": sd}, path)
    pol = ea.PointerNetworkPolicy()
    res = ea.load_reference_checkpoint(pol, str(path))
    assert not res.missing_keys and not res.unexpected_keys
    pol = pol.to(DEV).eval()
    with torch.no_grad():
        again = pol(td, env, phase="test", decode_type="greedy", return_sum_log_likelihood=False)
    assert torch.equal(again["actions"], out["actions"]) and torch.equal(again["log_likelihood"], out["log_likelihood"])


def test_evaluators():
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import eval as ev

    fx, env, td, out = rolled("ptrnet20_greedy")
    data = [ea.TensorDict({"locs": torch.from_numpy(fx["locs"])}, batch_size=[fx["locs"].shape[0]])]
    res = ev.GreedyEval(env)(policy(), data)
    assert np.array_equal(res["actions"].numpy(), fx["actions"])
    np.testing.assert_allclose(res["rewards"].numpy(), fx["reward"], rtol=1e-6)
    with pytest.raises(NotImplementedError, match="num_starts"):
        ev.GreedyMultiStartEval(env, num_starts=4)(policy(), data)
    with pytest.raises(NotImplementedError, match="num_starts"):
        ev.SamplingEval(env, samples=4)(policy(), data)


def test_a_graph_of_129_nodes_raises():
    env, td = make_td(torch.rand(2, 129, 2))
    with pytest.raises(NotImplementedError, match="2..128"):
        policy()(td, env, phase="test", decode_type="greedy")
