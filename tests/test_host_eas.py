"""CPU (no GPU needed): the host side of the EAS-Emb search (eam_rl4co_amd/search.py) -- the d loss / d log-likelihood rule
against autograd of the reference's loss, the C-ABI entry of the logit-key-only backward, and what the search refuses."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_loss(ll, reward, baseline, eas_lambda, incumbent):
    """zoo/eas/search.py:223-241 on ll / reward [B, n_aug, S + 1] (last column: the incumbent); without an incumbent group
    (iteration 0 here) [B, n_aug, S] and no imitation term."""
    group_reward = reward[..., :-1] if incumbent else reward
    if baseline == "multistart":
        bl_val = group_reward.mean(dim=-1, keepdim=True)
    elif baseline == "symmetric":
        bl_val = group_reward.mean(dim=-2, keepdim=True)
    else:
        bl_val = group_reward.mean(dim=-1, keepdim=True).mean(dim=-2, keepdim=True)
    advantage = group_reward - bl_val
    if not incumbent:
        return -(advantage * ll).mean()
    loss_rl = -(advantage * ll[..., :-1]).mean()
    loss_il = -ll[..., -1].mean()
    return loss_rl + eas_lambda * loss_il


@pytest.mark.parametrize("baseline", ["multistart", "symmetric", "full"])
@pytest.mark.parametrize("incumbent", [False, True])
@pytest.mark.parametrize("shape", [(3, 8, 7), (1, 2, 5), (2, 1, 4)])
def test_loss_coefficients_equal_autograd_of_the_reference_loss(baseline, incumbent, shape):
    from eam_rl4co_amd.search import eas_loss_coefficients

    g = torch.Generator().manual_seed(11)
    B, A, S = shape
    reward = -torch.rand(B, A, S + incumbent, generator=g, dtype=torch.float64) * 10
    ll = (-torch.rand(B, A, S + incumbent, generator=g, dtype=torch.float64) * 30).requires_grad_()
    lam = 0.013
    (ref,) = torch.autograd.grad(reference_loss(ll, reward, baseline, lam, incumbent), ll)
    got = eas_loss_coefficients(reward[..., :S], baseline, lam, incumbent)
    assert got.shape == ref.shape and got.dtype == torch.float64
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=0)


def test_backward_lp_is_declared_and_bound():
    from eam_rl4co_amd import _lib, ops

    with open(os.path.join(ROOT, "include", "eamrl.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+eamrl_reeval_backward_lp\s*\(\s*const\s+eamrl_reeval\s*\*\s*p\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert "eamrl_reeval_backward_lp" in _lib.PROTOTYPES
    lib = _lib.load()
    # its own argument check, before any launch: a null struct, then a graph above one key chunk and a dynamic embedding
    assert lib.eamrl_reeval_backward_lp(None, None) == -1
    assert b"eamrl_reeval_backward_lp" in lib.eamrl_last_error()
    s = _lib.Reeval()
    s.M = 113
    assert lib.eamrl_reeval_backward_lp(C.byref(s), None) == -1 and b"p->M <= 112" in lib.eamrl_last_error()
    s.M, s.dyn = 20, 1 << 12
    assert lib.eamrl_reeval_backward_lp(C.byref(s), None) == -1 and b"!p->dyn" in lib.eamrl_last_error()
    assert callable(ops.ReevalPlan.backward_lp)


def test_unsupported_searches_raise():
    import eam_rl4co_amd as ea

    env = ea.get_env("tsp", generator_params=dict(num_loc=10))
    pol = ea.AttentionModelPolicy(env_name="tsp").eval()
    with pytest.raises(NotImplementedError):
        ea.EASLay(env, pol)
    with pytest.raises(NotImplementedError):
        ea.EAS(env, pol, use_eas_layer=True)
    with pytest.raises(NotImplementedError):
        ea.EASEmb(env, pol, num_parallel_runs=2)
    with pytest.raises(NotImplementedError):
        ea.EASEmb(ea.get_env("pdp", generator_params=dict(num_loc=10)), ea.AttentionModelPolicy(env_name="pdp").eval())
    with pytest.raises(ValueError):
        ea.EASEmb(env, pol, eas_emb_cache_keys=["node_embeddings"])
    eas = ea.EAS(env, pol, use_eas_embedding=True, use_eas_layer=False)        # the same class as EASEmb
    assert isinstance(ea.EASEmb(env, pol), ea.EAS) and eas.keys == ["logit_key"] and eas.eas_lambda == 0.013
    assert eas.max_iters == 200 and eas.baseline == "multistart" and eas.optimizer_kwargs == {"lr": 0.0041, "weight_decay": 1e-6}


def test_search_on_a_cpu_tensordict_fails_loudly():
    import eam_rl4co_amd as ea

    env = ea.get_env("tsp", generator_params=dict(num_loc=10))
    pol = ea.AttentionModelPolicy(env_name="tsp").eval()
    before = {k: v.clone() for k, v in pol.state_dict().items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ea.EASEmb(env, pol).search(env.reset(batch_size=[2]), max_iters=1)
    assert all(torch.equal(v, before[k]) for k, v in pol.state_dict().items())
