"""CPU (no GPU needed): the host side of PPO -- `train.ppo_loss_terms` against autograd of the reference's expression
(rl4co/models/rl/ppo/ppo.py:177-209) in float64, the mini-batch-size rules (ppo.py:87-101,139-148), the critic baseline of
`train.reinforce_loss`, the C-ABI field of the entropy gradient (include/eamrl.h: eamrl_reeval.gent) and its refusals, and
what the new names refuse."""
import ctypes as C
import logging
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_terms(ll_sum, logprobs, reward, value_pred, entropy, cfg):
    """ppo.py:177-209 as written (sub_td["logprobs"] = logprobs, previous_reward = reward.view(-1, 1))."""
    previous_reward = reward.view(-1, 1)
    ratio = torch.exp(ll_sum - logprobs).view(-1, 1)
    adv = previous_reward - value_pred.detach()
    if cfg["normalize_adv"]:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    surrogate_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - cfg["clip_range"], 1 + cfg["clip_range"]) * adv).mean()
    value_loss = F.huber_loss(value_pred, previous_reward)
    loss = surrogate_loss + cfg["vf_lambda"] * value_loss - cfg["entropy_lambda"] * entropy.mean()
    return dict(loss=loss, surrogate_loss=surrogate_loss, value_loss=value_loss, entropy=entropy.mean())


@pytest.mark.parametrize("normalize_adv", [False, True])
@pytest.mark.parametrize("cfg", [dict(clip_range=0.2, vf_lambda=0.5, entropy_lambda=0.01),
                                 dict(clip_range=0.1, vf_lambda=1.3, entropy_lambda=0.0)])
def test_loss_terms_equal_autograd_of_the_reference_expression(cfg, normalize_adv):
    from eam_rl4co_amd.train import ppo_loss_terms

    cfg = dict(cfg, normalize_adv=normalize_adv)
    g = torch.Generator().manual_seed(5)
    b = 12
    ent0 = 20 + torch.randn(b, generator=g, dtype=torch.float64)
    logprobs, reward = -30 * torch.rand(b, generator=g, dtype=torch.float64), -10 * torch.rand(b, generator=g, dtype=torch.float64)
    res = []
    for fn in (reference_terms, lambda *a: ppo_loss_terms(*a[:5], **a[5])):
        # log-ratios from -0.6 to 0.6: rows inside and outside [1 - eps, 1 + eps]; values on both sides of the rewards (huber's
        # two branches: |value - reward| up to 3)
        ll = (logprobs + torch.linspace(-0.6, 0.6, b, dtype=torch.float64)).requires_grad_()
        value = (reward.view(-1, 1) + torch.linspace(-3, 3, b, dtype=torch.float64).view(-1, 1).roll(5, 0)).requires_grad_()
        ent = ent0.clone().requires_grad_()
        out = fn(ll, logprobs, reward, value, ent, cfg)
        out["loss"].backward()
        res.append((out, ll.grad, value.grad, ent.grad, ll.detach()))
    (ref, *gref, llv), (got, *ggot, _) = res
    ratio = torch.exp(llv - logprobs)
    assert ((ratio > 1 + cfg["clip_range"]) | (ratio < 1 - cfg["clip_range"])).any() and ((ratio - 1).abs() < cfg["clip_range"]).any()
    assert set(got) == {"loss", "surrogate_loss", "value_loss", "entropy"}
    for k in got:
        torch.testing.assert_close(got[k], ref[k], rtol=1e-12, atol=0)
    for a, r in zip(ggot, gref):
        assert float(r.abs().max()) > 0 or cfg["entropy_lambda"] == 0.0
        torch.testing.assert_close(a, r, rtol=1e-12, atol=0)
    # the reward may come as [b] or [b, 1]
    o2 = ppo_loss_terms(llv, logprobs, reward.view(-1, 1), res[0][0]["loss"].new_zeros(b, 1), torch.ones(b, dtype=torch.float64), **cfg)
    assert o2["loss"].shape == ()


def test_mini_batch_size_rules_and_warnings(caplog):
    from eam_rl4co_amd.train import _ppo_mini_batch_size, _ppo_resolve_mini_batch

    with caplog.at_level(logging.WARNING, logger="eam_rl4co_amd.train"):
        assert _ppo_mini_batch_size(0.25) == 0.25 and _ppo_mini_batch_size(1.0) == 1.0 and _ppo_mini_batch_size(64) == 64
        assert not caplog.records
        for bad in (0.0, -0.5, 1.5):
            caplog.clear()
            assert _ppo_mini_batch_size(bad) == 0.25
            assert len(caplog.records) == 1 and "Setting mini_batch_size to 0.25" in caplog.text
        for bad in (0, -3):
            caplog.clear()
            assert _ppo_mini_batch_size(bad) == 128
            assert len(caplog.records) == 1 and "Setting mini_batch_size to 128" in caplog.text
    with pytest.raises(ValueError, match="integer or a float"):
        _ppo_mini_batch_size("all")
    assert _ppo_resolve_mini_batch(0.25, 10) == 2 and _ppo_resolve_mini_batch(0.25, 512) == 128      # int(B * f)
    assert _ppo_resolve_mini_batch(128, 10) == 10 and _ppo_resolve_mini_batch(4, 10) == 4          # capped at B
    assert _ppo_resolve_mini_batch(1.0, 7) == 7


def test_ppo_step_partition_keeps_the_last_partial_mini_batch():
    import eam_rl4co_amd as ea

    env = ea.get_env("tsp", generator_params=dict(num_loc=10))
    pol = ea.AttentionModelPolicy(env_name="tsp")
    step = ea.PPOStep(pol, env, mini_batch_size=0.25, generator=torch.Generator().manual_seed(3))
    assert (step.clip_range, step.ppo_epochs, step.mini_batch_size, step.vf_lambda, step.entropy_lambda, step.normalize_adv,
            step.max_grad_norm) == (0.2, 2, 0.25, 0.5, 0.0, False, 0.5)               # ppo.py:61-111
    assert isinstance(step.critic, ea.CriticNetwork) and isinstance(step.optimizer, torch.optim.Adam)
    assert step.optimizer.param_groups[0]["lr"] == 1e-4
    n_opt = sum(p.numel() for g in step.optimizer.param_groups for p in g["params"])
    assert n_opt == sum(p.numel() for p in pol.parameters()) + sum(p.numel() for p in step.critic.parameters())
    parts = step.partition(10)
    assert [len(p) for p in parts] == [2, 2, 2, 2, 2] and sorted(torch.cat(parts).tolist()) == list(range(10))
    parts = step.partition(11)
    assert [len(p) for p in parts] == [2, 2, 2, 2, 2, 1] and sorted(torch.cat(parts).tolist()) == list(range(11))
    again = ea.PPOStep(pol, env, mini_batch_size=0.25, generator=torch.Generator().manual_seed(3))
    assert [p.tolist() for p in again.partition(10) + again.partition(11)] == \
        [p.tolist() for p in ea.PPOStep(pol, env, generator=torch.Generator().manual_seed(3)).partition(10)] + [p.tolist() for p in parts]


def test_reinforce_loss_with_the_critic_baseline():
    """CriticBaseline.eval (baselines.py:140-159): bl = v.detach(), bl_loss = mse(v, reward), loss = reinforce_loss + bl_loss."""
    from eam_rl4co_amd import train

    reward = torch.tensor([-3.0, -5.0, -4.0])
    logp = torch.tensor([[-1.0, -2.0], [-0.5, -0.25], [-3.0, 0.0]], requires_grad=True)
    w = torch.tensor([0.5], requires_grad=True)

    class StubPolicy:
        def __call__(self, td, env, **kw):
            assert kw["phase"] == "train" and kw["return_sum_log_likelihood"] is False
            return {"actions": torch.zeros(3, 2, dtype=torch.int64), "reward": reward, "log_likelihood": logp}

    critic = lambda td: (w * td["x"]).view(-1, 1)
    td = {"x": torch.tensor([-5.0, -9.0, -8.5])}
    out = train.reinforce_loss(StubPolicy(), None, td, baseline="critic", critic=critic)
    v = 0.5 * td["x"]
    ll = logp.detach().sum(1)
    expect = -((reward - v) * ll).mean() + F.mse_loss(v, reward)
    torch.testing.assert_close(out["loss"].detach(), expect)
    torch.testing.assert_close(out["bl_val"], v)
    out["loss"].backward()
    torch.testing.assert_close(logp.grad, (-(reward - v) / 3)[:, None].expand(3, 2))          # the baseline is detached ...
    torch.testing.assert_close(w.grad, (2 * (v - reward) * td["x"]).mean().view(1))             # ... the critic learns from the mse
    with pytest.raises(ValueError, match="critic="):
        train.reinforce_loss(StubPolicy(), None, td, baseline="critic")
    with pytest.raises(NotImplementedError):
        train.reinforce_loss(StubPolicy(), None, td, baseline="critic", critic=critic, num_starts=4)
    # the other baselines are what they were
    out = train.reinforce_loss(StubPolicy(), None, td, baseline="mean")
    torch.testing.assert_close(out["loss"].detach(), -((reward - reward.mean()) * ll).mean())
    out = train.reinforce_loss(StubPolicy(), None, td, baseline="no")
    torch.testing.assert_close(out["loss"].detach(), -(reward * ll).mean())


def test_gent_is_the_last_member_of_the_struct_and_refused_where_it_is_not_built():
    from eam_rl4co_amd import _lib

    with open(os.path.join(ROOT, "include", "eamrl.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+eamrl_reeval\s*\{(.*?)\}\s*eamrl_reeval\s*;", text, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert re.fullmatch(r"const\s+float\s*\*\s*gent", decls[-1]), decls[-1]
    assert _lib.Reeval._fields_[-1] == ("gent", C.c_void_p)
    assert [n for n, _ in _lib.Reeval._fields_].count("gent") == 1 and _lib.Reeval.gent.offset + 8 == C.sizeof(_lib.Reeval)

    # the entry's checks, before any launch (no GPU is touched: every pointer below is a made-up aligned address)
    lib = _lib.load()
    p = 1 << 20
    keep = (C.c_char * 16)()

    def plan(M):
        s = _lib.Reeval()
        for name in ("K", "V", "Lp", "Pa", "idxA", "maskbits", "actions", "logp", "lse", "glogp", "dheads", "dK", "dV", "dLp", "dPa",
                     "entropy", "gent"):
            setattr(s, name, p)
        s.ld = s.ldg = 128
        s.B, s.R, s.S, s.T, s.M, s.nchunk, s.temp, s.clip = 2, 2, 1, 3, M, 1, 1.0, 10.0
        return s

    s = plan(20)
    s.entropy = None
    assert lib.eamrl_reeval_backward(C.byref(s), None) == -1
    assert b"eamrl_reeval_backward" in lib.eamrl_last_error() and b"p->entropy && p->lse" in lib.eamrl_last_error()
    s = plan(20)
    s.lse = None
    assert lib.eamrl_reeval_backward(C.byref(s), None) == -1 and b"p->entropy && p->lse" in lib.eamrl_last_error()
    s = plan(113)           # key chunks
    s.scratch, s.nkc = p, 2
    assert lib.eamrl_reeval_backward(C.byref(s), None) == -1 and b"p->M <= 112" in lib.eamrl_last_error()
    del keep


def test_unsupported_constructions_raise():
    import eam_rl4co_amd as ea

    env = ea.get_env("tsp", generator_params=dict(num_loc=10))
    pol = ea.AttentionModelPolicy(env_name="tsp")
    with pytest.raises(NotImplementedError):
        ea.CriticNetwork(pol.encoder, customized=True)
    with pytest.raises(NotImplementedError):
        ea.CriticNetwork(torch.nn.Linear(2, 128))
    with pytest.raises(NotImplementedError):
        ea.create_critic_from_actor(ea.HeterogeneousAttentionModelPolicy(env_name="pdp"))       # not an AttentionModelEncoder
    with pytest.raises(ValueError, match="backbone"):
        ea.create_critic_from_actor(pol, backbone="trunk")
    with pytest.raises(NotImplementedError, match="PolyNet"):
        ea.PPOStep(ea.PolyNetPolicy(k=4, env_name="tsp"), env)
    critic = ea.create_critic_from_actor(pol, hidden_dim=256)
    assert critic.encoder is not pol.encoder and critic.value_head[0].weight.shape == (256, 128)
    assert [k for k in critic.state_dict() if not k.startswith("encoder.")] == \
        ["value_head.0.weight", "value_head.0.bias", "value_head.2.weight", "value_head.2.bias"]
    from eam_rl4co_amd.train import evaluate_log_likelihood

    with pytest.raises(NotImplementedError, match="top_k / top_p"):
        evaluate_log_likelihood(pol, None, env, torch.zeros(2, 10, dtype=torch.int64), top_k=3, return_entropy=True)


def test_a_cpu_tensordict_has_no_fallback_and_changes_nothing():
    import eam_rl4co_amd as ea

    env = ea.get_env("tsp", generator_params=dict(num_loc=10))
    pol = ea.AttentionModelPolicy(env_name="tsp")
    step = ea.PPOStep(pol, env)
    before = [{k: v.clone() for k, v in m.state_dict().items()} for m in (pol, step.critic)]
    td = env.reset(batch_size=[4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        step(td)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        step.critic(td)
    for m, b in zip((pol, step.critic), before):
        assert all(torch.equal(v, b[k]) for k, v in m.state_dict().items())
