"""GPU: PPO (eam_rl4co_amd/train.py: ppo_loss_terms, PPOStep; eam_rl4co_amd/critic.py) on the native kernels.

  critic            value and the gradient of every critic parameter against a float64 torch restatement of
                    rl4co/models/rl/common/critic.py:57-59 (`critic_restated`: encoder and value head spelled out in torch ops);
                    state-dict keys against the contract recorded from the reference (golden/state_dict_contract_critic.json)
  fixtures          one PPO mini-batch (rl4co/models/rl/ppo/ppo.py:168-209 at entropy_lambda 0.01, vf_lambda 0.5, clip_range 0.2)
                    against values and gradients recorded from the reference itself (golden/make_golden_ppo.py -> ppo_*.npz), with the train fixtures' tolerances (tests/test_gpu_train.py:73-108)
  native / PyTorch  the gradient of one mini-batch through the native re-evaluation (entropy gradient in the backward kernel)
                    against EAMRL_NATIVE_REEVAL=0 (PyTorch autograd), and the same for the entropy alone
  PPOStep           mini-batch partition, determinism under a seeded generator, both networks move, ratio 1 at the first
                    mini-batch, graph-carrying entropy

Tolerance of the native-versus-autograd comparisons: values within 1e-4 max|ref|; gradients by the rule of
test_native_reevaluation_matches_autograd (tests/test_gpu_train.py:605-618), see `compare_grads`.

PPOStep, same seed twice: the partition, the rollout and the first mini-batch's forward values are bit-identical.  The
parameters after the step are NOT guaranteed to be: the backward kernels of the re-evaluation add their partial sums with float
atomics in arrival order (two calls of `ReevalPlan.backward` on the same inputs differ in the last bits: measured on the
MI355X, and so did the parameters of two CVRP runs, by at most 6e-8, while TSP and PDP came out equal).  They are therefore held
to what the gradient contract implies for plain SGD, see test_ppo_step_is_reproducible.
"""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import goldweights
import pdp_ref
from _util import GOLDEN, cfg_for, golden, instance_of
from test_gpu_parity import DEV, make_policy, make_td, t

pytestmark = pytest.mark.gpu

CLIP_RANGE, VF_LAMBDA, ENTROPY_LAMBDA = 0.2, 0.5, 0.01


# ---- setup ---------------------------------------------------------------------------------------------------------------------
def policy_for(cfg):
    """The policies of the training tests: closed-form weights; batch norm in train() mode (am_*), instance norm (pomo_*)."""
    if cfg.endswith("_pdp"):
        import eam_rl4co_amd as ea

        pol = ea.AttentionModelPolicy(env_name="pdp").eval()
        sd = pol.state_dict()
        for k, v in pdp_ref.weights(cfg).items():
            sd[k].copy_(torch.from_numpy(v))
        return pol.to(DEV).train()
    return make_policy(cfg).train()


def critic_for(pol):
    """create_critic_from_actor + the closed-form streams of `value_head.*` (the copied encoder keeps the policy's values)."""
    import eam_rl4co_amd as ea

    critic = ea.create_critic_from_actor(pol)
    sd = critic.state_dict()
    for k, v in sd.items():
        if k.startswith("value_head."):
            v.copy_(torch.from_numpy(goldweights.tensor_for(k, tuple(v.shape))))
    return critic


def instances(env_name, B, seed=5):
    import eam_rl4co_amd as ea

    env = ea.get_env(env_name, generator_params=dict(num_loc=20), seed=seed)
    torch.manual_seed(seed)
    return env, env.reset(batch_size=[B]).to(DEV)


SETUPS = [("am_tsp", "tsp", 8), ("am_cvrp", "cvrp", 8), ("pomo_tsp", "tsp", 8), ("am_pdp", "pdp", 4)]


def close(got, ref, what=""):
    """A value tensor: |got - ref| <= 1e-4 max|ref|."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale, err = float(ref.abs().max()), float((got - ref).abs().max())
    print(f"PPO {what}: max-abs error {err:.3e} / max|ref| {scale:.3e} = {err / scale:.2e}")
    assert err <= 1e-4 * scale, (what, err, scale)


def compare_grads(got: dict, ref: dict, what):
    """The gradient rule of test_native_reevaluation_matches_autograd (tests/test_gpu_train.py:605-618), unchanged: per tensor
    the norm of the difference within 1e-4 of the reference's norm, and no element further than 5e-4 of the tensor's largest;
    a tensor whose gradient is rounding noise (a bias in front of a batch norm: true gradient 0) is measured against 1e-2 of
    the global gradient norm / of the largest element of all."""
    assert got.keys() == ref.keys()
    ref = {k: v.detach().double().cpu() for k, v in ref.items()}
    gnorm = float(torch.sqrt(sum((g ** 2).sum() for g in ref.values())))
    top = max(float(g.abs().max()) for g in ref.values())
    bad = []
    for k, r in ref.items():
        g = got[k].detach().double().cpu()
        rel = float((g - r).norm()) / max(float(r.norm()), 1e-2 * gnorm)
        el = float((g - r).abs().max()) / max(float(r.abs().max()), 1e-2 * top)
        print(f"PPO {what} d{k}: norm-wise {rel:.2e} (bound 1e-4), element-wise {el:.2e} (bound 5e-4)")
        if not (rel <= 1e-4 and el <= 5e-4):
            bad.append((k, rel, el))
    assert bad == []


# ---- critic ----------------------------------------------------------------------------------------------------------------------
def critic_restated(critic, td):
    """critic.py:57-59 in plain torch ops, in the dtype of `critic`: h, _ = encoder(td); value_head(h).mean(1).
    Encoder: init embedding (nn/env_embeddings/init.py) -> layers of {h + MHA(h), norm, h + FFN(h), norm}
    (nn/graph/attnnet.py:12-60, nn/attention.py:112-136, nn/ops.py:34-53; batch norm with batch statistics in train() mode)."""
    enc, env_name = critic.encoder, critic.encoder.env_name
    ie = enc.init_embedding
    dt = next(critic.parameters()).dtype
    locs = td["locs"].to(dt)
    if env_name == "tsp":
        h = F.linear(locs, ie.init_embed.weight, ie.init_embed.bias)
    elif env_name == "pdp":
        half = (locs.shape[1] - 1) // 2
        pick, deliv = locs[:, 1:half + 1], locs[:, half + 1:]
        h = torch.cat((F.linear(locs[:, :1], ie.init_embed_depot.weight, ie.init_embed_depot.bias),
                       F.linear(torch.cat((pick, deliv), -1), ie.init_embed_pick.weight, ie.init_embed_pick.bias),
                       F.linear(deliv, ie.init_embed_delivery.weight, ie.init_embed_delivery.bias)), 1)
    else:
        feat = torch.cat((locs[:, 1:], td["demand"].to(dt)[..., None]), -1)
        h = torch.cat((F.linear(locs[:, :1], ie.init_embed_depot.weight, ie.init_embed_depot.bias),
                       F.linear(feat, ie.init_embed.weight, ie.init_embed.bias)), 1)

    def norm(layer, x):
        n = layer.normalizer
        if isinstance(n, torch.nn.BatchNorm1d):
            assert critic.training
            return F.batch_norm(x.reshape(-1, x.shape[-1]), None, None, n.weight, n.bias, True, 0.0, n.eps).view_as(x)
        return F.instance_norm(x.permute(0, 2, 1), weight=n.weight, bias=n.bias, eps=n.eps).permute(0, 2, 1)

    for layer in enc.net.layers:
        mha, ffn = layer[0].module, layer[2].module
        B, N, E = h.shape
        H = mha.num_heads
        q, k, v = F.linear(h, mha.Wqkv.weight, mha.Wqkv.bias).view(B, N, 3, H, E // H).permute(2, 0, 3, 1, 4)
        a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(E // H), -1)
        att = (a @ v).permute(0, 2, 1, 3).reshape(B, N, E)
        h = norm(layer[1], h + F.linear(att, mha.out_proj.weight, mha.out_proj.bias))
        x = h
        for lin in ffn.lins[:-1]:
            x = F.relu(F.linear(x, lin.weight, lin.bias))
        h = norm(layer[3], h + F.linear(x, ffn.lins[-1].weight, ffn.lins[-1].bias))
    return critic.value_head(h).mean(1)


@pytest.mark.parametrize("cfg,env_name,B", SETUPS)
def test_critic_value_and_gradients_match_the_float64_restatement(cfg, env_name, B):
    env, td = instances(env_name, B)
    critic = critic_for(policy_for(cfg))
    c64 = copy.deepcopy(critic).double()
    w = torch.randn(B, 1, generator=torch.Generator().manual_seed(1)).to(DEV)
    v64 = critic_restated(c64, td)
    (v64 * w.double()).sum().backward()
    ref = {k: p.grad for k, p in c64.named_parameters()}
    with torch.no_grad():
        v_nograd = critic(td)                       # the encoder's own forward (fused kernel where it applies)
    v = critic(td)                                  # the training graph on the native autograd functions
    assert v.shape == (B, 1) and v.grad_fn is not None and v_nograd.grad_fn is None
    (v * w).sum().backward()
    close(v_nograd, v64, what=f"{cfg} value (no grad)")
    close(v, v64, what=f"{cfg} value")
    compare_grads({k: p.grad for k, p in critic.named_parameters()}, ref, cfg)


def test_critic_state_dict_keys_are_the_references():
    with open(os.path.join(GOLDEN, "state_dict_contract_critic.json")) as f:
        contract = json.load(f)
    for cfg in ("am_tsp", "am_cvrp"):
        sd = critic_for(policy_for(cfg)).state_dict()
        got = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]
        assert got == contract["critic_" + cfg]
        assert {"value_head.0.weight", "value_head.0.bias", "value_head.2.weight", "value_head.2.bias"} <= set(sd)


# ---- the reference's own numbers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ppo_tsp20", "ppo_cvrp20"])
def test_fixture_has_clipped_and_unclipped_rows(name):
    """(CPU arithmetic on the recorded numbers: the surrogate of the fixture exercises both branches of the min)"""
    fx = golden(name)
    ratio, adv = fx["ratio"].reshape(-1), (fx["reward"].reshape(-1, 1) - fx["value"]).reshape(-1)
    clipped = np.clip(ratio, 1 - CLIP_RANGE, 1 + CLIP_RANGE) * adv < ratio * adv
    assert clipped.any() and (~clipped).any() and np.array_equal(clipped, fx["took_clipped"])
    outside = (ratio < 1 - CLIP_RANGE) | (ratio > 1 + CLIP_RANGE)
    assert outside.any() and (~outside).any()
    assert float(fx["entropy_lambda"]) == ENTROPY_LAMBDA and float(fx["vf_lambda"]) == VF_LAMBDA and float(fx["clip_range"]) == CLIP_RANGE


def _fixture_mini_batch(name):
    import eam_rl4co_amd as ea

    fx = golden(name)
    env_name = str(fx["env_name"])
    pol = policy_for(cfg_for(fx))
    critic = critic_for(pol)
    env, td = make_td(env_name, fx["locs"], instance_of(fx))
    step = ea.PPOStep(pol, env, critic=critic, clip_range=CLIP_RANGE, vf_lambda=VF_LAMBDA, entropy_lambda=ENTROPY_LAMBDA)
    terms = step.mini_batch_terms(td, t(fx["actions"]), t(fx["ll_old"], torch.float32), t(fx["reward"]))
    return fx, pol, critic, step, terms


@pytest.mark.parametrize("name", ["ppo_tsp20", "ppo_cvrp20"])
def test_mini_batch_values_match_the_reference(name):
    fx, pol, critic, step, terms = _fixture_mini_batch(name)
    np.testing.assert_allclose(terms["ll"].detach().cpu().numpy(), fx["ll"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(terms["entropy_rows"].detach().cpu().numpy(), fx["entropy"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(terms["value"].detach().cpu().numpy(), fx["value"], rtol=2e-5, atol=2e-5)
    for k in ("loss", "surrogate_loss", "value_loss"):
        np.testing.assert_allclose(float(terms[k].detach()), float(fx[k]), rtol=2e-5, err_msg=k)
    np.testing.assert_allclose(float(terms["entropy"].detach()), float(fx["entropy"].mean()), rtol=2e-5)
    assert terms["entropy_rows"].grad_fn is not None and terms["ll"].grad_fn is not None


@pytest.mark.parametrize("name", ["ppo_tsp20", "ppo_cvrp20"])
def test_mini_batch_gradients_match_the_reference(name):
    """Every parameter of policy and critic, by the rule of the train fixtures (tests/test_gpu_train.py:98-109): the norm of
    each gradient within 1e-4 max(reference norm, 1e-3 of the total gradient norm), every element of the small tensors within
    1e-4 max(largest reference element, 1e-3 of the total).

    The fixtures' own condition (golden/make_golden_ppo.py): a data seed is used only if the reference's own float32 gradients
    lie within this very tolerance of its float64 run -- the gradients that vanish by cancellation through the first batch norm
    are pure rounding at 1e-7 of the total gradient norm, the floor of the rule, in the reference as here.
    Measured on the MI355X (two runs): the closest tensors are those two -- ppo_tsp20 init_embed.bias at 0.87 of its bound
    (4.005e-05 against 4.604e-05) and layer 0's out_proj.bias at 0.75, the same figures in both runs; ppo_cvrp20's worst is that
    out_proj.bias at 0.28 and 0.46 (the float atomics of the backward differ from run to run); every other tensor below 0.5."""
    fx, pol, critic, step, terms = _fixture_mini_batch(name)
    step.grads.zero_()
    terms["loss"].backward()
    bad = []
    for tag, module in (("policy", pol), ("critic", critic)):
        params = dict(module.named_parameters())
        names, norms = fx[f"{tag}_grad_names"], fx[f"{tag}_grad_norms"]
        assert sorted(str(k) for k in names) == sorted(params)
        total_ref = float(np.sqrt((norms ** 2).sum()))
        for k, ref_norm in zip(names, norms):
            g = params[str(k)].grad
            got = 0.0 if g is None else float(g.double().norm())
            bd = 1e-4 * max(ref_norm, 1e-3 * total_ref) + 1e-7
            print(f"PPO {name} {tag} |d{k}|: {got:.6e} against {ref_norm:.6e}: {abs(got - ref_norm):.3e}, bound {bd:.3e}")
            if not abs(got - ref_norm) <= bd:
                bad.append((tag, str(k), "norm", abs(got - ref_norm), bd))
            key = f"{tag}_grad__{k}"
            if key in fx and g is not None:
                ref = fx[key]
                atol = 1e-4 * max(float(np.abs(ref).max()), 1e-3 * total_ref)
                err = float(np.abs(g.cpu().numpy() - ref).max())
                print(f"PPO {name} {tag} d{k}: largest element error {err:.3e}, bound {atol:.3e}")
                if not err <= atol:
                    bad.append((tag, str(k), "element", err, atol))
    assert any(str(k).startswith("value_head.") for k in fx["critic_grad_names"])
    assert bad == []


# ---- native re-evaluation against the PyTorch path ------------------------------------------------------------------------------
def _rollout(pol, env, td):
    with torch.no_grad():
        out = pol(td.clone(), env, phase="train")
    return out["actions"].contiguous(), out["reward"], out["log_likelihood"]


def _grads(module):
    return {k: p.grad.clone() for k, p in module.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("cfg,env_name,B", SETUPS[:3])
@pytest.mark.parametrize("what", ["mini_batch", "entropy_only"])
def test_native_mini_batch_gradient_equals_the_pytorch_path(cfg, env_name, B, what, monkeypatch):
    import eam_rl4co_amd as ea
    from eam_rl4co_amd.train import native_reeval_supported

    env, td = instances(env_name, B)
    pol = policy_for(cfg)
    critic = critic_for(pol)
    step = ea.PPOStep(pol, env, critic=critic, clip_range=CLIP_RANGE, vf_lambda=VF_LAMBDA, entropy_lambda=ENTROPY_LAMBDA)
    actions, reward, ll_old = _rollout(pol, env, td)
    ll_old = ll_old + torch.tensor([0.5, -0.5, 0.05, -0.05, 0.3, -0.3, 0.1, -0.1], device=DEV)[:B]      # clipped and unclipped rows
    res = []
    for native in ("1", "0"):
        monkeypatch.setenv("EAMRL_NATIVE_REEVAL", native)
        assert native_reeval_supported(pol, td["locs"].shape[1]) == (native == "1")
        terms = step.mini_batch_terms(td, actions, ll_old, reward)
        step.grads.zero_()
        (terms["loss"] if what == "mini_batch" else terms["entropy_rows"].mean()).backward()
        res.append((terms, _grads(pol)))
    (tn, gn), (tt, gt) = res
    assert float(sum(g.abs().sum() for g in gt.values())) > 0
    close(tn["ll"], tt["ll"], what=f"{cfg} ll")
    close(tn["entropy_rows"], tt["entropy_rows"], what=f"{cfg} entropy")
    compare_grads(gn, gt, f"{cfg} {what}")


# ---- PPOStep -------------------------------------------------------------------------------------------------------------------
PPO_ENVS = [("am_tsp", "tsp"), ("am_cvrp", "cvrp"), ("am_pdp", "pdp")]


def _fresh_step(cfg, env, sgd=False):
    import eam_rl4co_amd as ea

    pol = policy_for(cfg)
    critic = critic_for(pol)
    opt = torch.optim.SGD(list(pol.parameters()) + list(critic.parameters()), lr=1e-4) if sgd else None
    step = ea.PPOStep(pol, env, critic=critic, mini_batch_size=0.25, ppo_epochs=2, entropy_lambda=ENTROPY_LAMBDA, optimizer=opt,
                      generator=torch.Generator().manual_seed(77))
    seen = []
    inner = step.partition
    step.partition = lambda n: seen.append(inner(n)) or seen[-1]
    return pol, critic, step, seen


@pytest.mark.parametrize("cfg,env_name", PPO_ENVS)
def test_ppo_step_partitions_the_batch_and_moves_both_networks(cfg, env_name):
    B = 10 if env_name != "pdp" else 4
    env, td = instances(env_name, B, seed=9)
    pol, critic, step, seen = _fresh_step(cfg, env)
    before = [copy.deepcopy(pol.state_dict()), copy.deepcopy(critic.state_dict())]
    out = step(td)
    mb = int(B * 0.25)
    assert out["optimizer_steps"] == 2 * -(-B // mb) and (B != 10 or out["optimizer_steps"] == 10)
    assert len(seen) == 2
    for epoch in seen:                          # every instance once per epoch, the last partial mini-batch kept
        assert sorted(torch.cat(epoch).tolist()) == list(range(B)) and all(len(i) <= mb for i in epoch)
    assert all(torch.isfinite(out[k]).all() for k in ("loss", "surrogate_loss", "value_loss", "entropy"))
    assert out["actions"].shape[0] == B and out["reward"].shape == (B,)
    moved = [any(not torch.equal(v, b[k]) for k, v in m.state_dict().items() if k.endswith("weight"))
             for m, b in zip((pol, critic), before)]
    assert moved == [True, True]


@pytest.mark.parametrize("cfg,env_name", PPO_ENVS)
def test_ppo_step_is_reproducible(cfg, env_name):
    """Two fresh copies, the same generator seed and the same sampling seed: the same partition, the same tours, bit for bit
    the same forward values of the first mini-batch.  Parameters after the step (plain SGD, lr 1e-4, so that the update is
    linear in the gradient): each of the n optimizer steps applies a gradient clipped to max_grad_norm = 0.5 that the
    re-evaluation contract holds to 1e-4 of its norm, so two runs that differ only in the order of float atomics end within
    n * lr * 2 * 1e-4 * 0.5 of each other in norm (a different partition or tour would move them apart by about n * lr * 0.5).
    Measured: 0 for TSP and PDP, 1.7e-8 for CVRP (a handful of parameters one float32 ulp apart) against the bound of 1e-7."""
    B = 10 if env_name != "pdp" else 4
    env, td = instances(env_name, B, seed=9)
    runs = []
    for _ in range(2):
        pol, critic, step, seen = _fresh_step(cfg, env, sgd=True)
        torch.manual_seed(3)                        # the rollout's sampling
        actions, reward, ll_old = _rollout(pol, env, td)
        idx = torch.arange(B)[:max(int(B * 0.25), 1)]
        terms = step.mini_batch_terms(td[idx], actions[idx.to(DEV)].contiguous(), ll_old[idx.to(DEV)], reward[idx.to(DEV)])
        first = [terms[k].detach().clone() for k in ("ll", "entropy_rows", "value", "loss")]
        torch.manual_seed(3)
        out = step(td)
        flat = torch.cat([p.detach().double().reshape(-1) for m in (pol, critic) for p in m.parameters()])
        runs.append((seen, actions, reward, first, out, flat))
    a, b = runs
    assert [i.tolist() for e in a[0] for i in e] == [i.tolist() for e in b[0] for i in e]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[4]["actions"], b[4]["actions"])
    assert all(torch.equal(x, y) for x, y in zip(a[3], b[3]))
    n = a[4]["optimizer_steps"]
    dist = float((a[5] - b[5]).norm())
    print(f"PPO {cfg}: parameters of the two runs differ by {dist:.3e} in norm after {n} SGD steps (bound {n * 1e-4 * 1e-4:.1e})")
    assert dist <= n * 1e-4 * 2 * 1e-4 * 0.5


def test_first_mini_batch_ratio_is_one_with_an_instance_norm_policy():
    """Nothing has been updated yet and instance norm does not depend on the batch: the re-evaluated log-likelihood of a
    mini-batch is the rollout's, 1e-5 per step over 20 steps."""
    import eam_rl4co_amd as ea

    env, td = instances("tsp", 10)
    pol = policy_for("pomo_tsp")
    step = ea.PPOStep(pol, env, critic=critic_for(pol), entropy_lambda=ENTROPY_LAMBDA, generator=torch.Generator().manual_seed(1))
    actions, reward, ll_old = _rollout(pol, env, td)
    idx = step.partition(10)[0]
    sub, idx = td[idx], idx.to(DEV)
    terms = step.mini_batch_terms(sub, actions[idx].contiguous(), ll_old[idx], reward[idx])
    ratio = torch.exp(terms["ll"].sum(-1) - ll_old[idx])
    print("PPO first mini-batch ratio - 1:", (ratio - 1).abs().max().item())
    assert float((ratio - 1).abs().max()) <= 1e-3


@pytest.mark.parametrize("cfg,env_name,B", SETUPS)
def test_entropy_of_given_tours_carries_a_graph_only_under_autograd(cfg, env_name, B):
    from eam_rl4co_amd.train import native_reeval_supported

    env, td = instances(env_name, B)
    pol = policy_for(cfg).eval()                    # (eval: the two calls see the same normalisation statistics)
    actions = _rollout(pol, env, td)[0]
    with torch.no_grad():
        plain = pol(td.clone(), env, phase="train", actions=actions, return_entropy=True)
    seen = []
    if native_reeval_supported(pol, td["locs"].shape[1]):       # the value the call computes: `_native_entropy`'s, detached
        inner = pol._native_entropy
        pol._native_entropy = lambda *a: seen.append(inner(*a)) or seen[-1]
    out = pol(td.clone(), env, phase="train", actions=actions, return_entropy=True)
    assert plain["entropy"].grad_fn is None and out["entropy"].grad_fn is not None and out["entropy"].shape == (B,)
    for v in seen:
        assert v.grad_fn is None and torch.equal(out["entropy"].detach(), v)
    # ... which is the no-grad call's up to the contract of the re-evaluation (1e-5 per step: under autograd the kernel is
    # handed the rollout's glimpse outputs, without it recomputes them)
    T = actions.shape[1]
    np.testing.assert_allclose(out["entropy"].detach().cpu().numpy(), plain["entropy"].cpu().numpy(), rtol=0, atol=1e-5 * T)
    sampled = pol(td.clone(), env, phase="train", return_entropy=True)
    assert sampled["entropy"].grad_fn is None and sampled["log_likelihood"].grad_fn is not None
    out["entropy"].sum().backward()
    assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in pol.parameters())
