#!/usr/bin/env python3
"""Generate the PPO golden vectors tests/golden/ppo_*.npz by RUNNING THE REFERENCE.

    python tests/golden/make_golden_ppo.py

Same machinery as make_golden.py's train cases (reference modules through `_refshim`, closed-form `goldweights`): the reference's
AttentionModelPolicy in train() mode (BatchNorm: batch statistics) and its CriticNetwork from `create_critic_from_actor`
(rl4co/models/rl/common/critic.py:13-77; the value head filled from the `goldweights` streams of `value_head.*`, the copied
encoder keeps the policy's values, which are the streams of `encoder.*`).  The PPO trainer class needs Lightning (absent), so
the lines of its inner loop (rl4co/models/rl/ppo/ppo.py:131-134 for the rollout, 168-209 for one mini-batch) are applied here to
the reference policy's and critic's own outputs, with the whole batch as the mini-batch:

    no_grad: out = policy(td.clone(), env, phase="train")                      -> actions, reward, old log-likelihood
    out = policy(sub_td.clone(), actions=..., env=env, return_entropy=True, return_sum_log_likelihood=False)
    ratio, adv, surrogate_loss, value_loss, loss                                at clip_range 0.2, vf_lambda 0.5, entropy_lambda 0.01

Everything is recorded in float32, as the reference trains and as the train fixtures are recorded.  One condition of its
own, applied HERE and not in the tests (as make_golden_pdp.py does with near ties): a data seed is used only if the reference's
own float32 gradients lie within the fixtures' tolerance of its float64 run (`run_ppo_case`).

The old log-likelihood is PERTURBED by a fixed pattern before the ratio is taken (the policy has not changed between the two
passes, so the true ratio is 1 everywhere): the script asserts that at least one row's surrogate takes the clipped branch and
at least one the unclipped one.  Stored: the instance, actions, reward, the (perturbed) old log-likelihood, the reference's
per-step log-likelihood, entropy, critic value, the three loss terms and the total, and the gradients of the policy's parameters
(norm; full tensors for the small ones, as the train fixtures) and of the critic's `value_head.*` and encoder.
Also writes state_dict_contract_critic.json: the key names, shapes and dtypes of the reference critic's state_dict.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refshim  # noqa: E402,F401  (make_golden installs it)
import goldweights  # noqa: E402
from make_golden import gen_params, make_policy, np_  # noqa: E402

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import copy  # noqa: E402
import importlib.util  # noqa: E402
import types  # noqa: E402

from tensordict import TensorDict  # noqa: E402  (the stand-in of _refshim)

from rl4co.envs.routing.cvrp.env import CVRPEnv  # noqa: E402
from rl4co.envs.routing.tsp.env import TSPEnv  # noqa: E402

# rl4co/models/rl/__init__.py imports the Lightning trainers (absent); critic.py itself is a plain file: skip the two package
# __init__s on the way to it, as `_refshim.install` does for rl4co.models.common / .zoo
for _pkg in ("rl4co.models.rl", "rl4co.models.rl.common"):
    if _pkg not in sys.modules:
        _m = types.ModuleType(_pkg)
        _m.__path__ = [importlib.util.find_spec("rl4co").submodule_search_locations[0] + "/" + "/".join(_pkg.split(".")[1:])]
        sys.modules[_pkg] = _m

from rl4co.models.rl.common.critic import create_critic_from_actor  # noqa: E402

CLIP_RANGE, VF_LAMBDA, ENTROPY_LAMBDA = 0.2, 0.5, 0.01
# added to the rollout's log-likelihood, row i gets PERTURB[i % 8]: log(1.2) = 0.182, so +-0.5 / +-0.3 leave the ratio outside
# [0.8, 1.2] and +-0.05 / +-0.1 inside
PERTURB = (0.5, -0.5, 0.05, -0.05, 0.3, -0.3, 0.1, -0.1)


SEEDS_TRIED = 16


def own_rounding(r32, r64):
    """The reference's float32 gradients measured against its float64 run BY THE RULE THE FIXTURE IS MATCHED WITH
    (tests/test_gpu_train.py:98-109: norms within 1e-4 max(norm, 1e-3 total), elements of the small tensors within 1e-4
    max(largest element, 1e-3 total)): -> (largest error / bound over all recorded tensors, its name)."""
    worst = (0.0, "")
    for tag in ("pol", "cri"):
        p32, p64 = dict(r32[tag].named_parameters()), dict(r64[tag].named_parameters())
        total = float(np.sqrt(sum(float(p.grad.double().norm()) ** 2 for p in p32.values() if p.grad is not None)))
        for k, p in p32.items():
            if p.grad is None:
                continue
            n32, g64 = float(p.grad.double().norm()), p64[k].grad
            worst = max(worst, (abs(n32 - float(g64.norm())) / (1e-4 * max(n32, 1e-3 * total) + 1e-7), f"|{k}|"))
            if p.numel() <= 512:
                bound = 1e-4 * max(float(p.grad.abs().max()), 1e-3 * total)
                worst = max(worst, (float((p.grad.double() - g64).abs().max()) / bound, k))
    return worst


def run_ppo_case(name, env_name, num_loc, batch, first_seed):
    """Walks the data seeds from `first_seed` to the first one whose recorded numbers are fit to be matched with the fixtures'
    tolerance: the reference's OWN float32 gradients must lie within that tolerance of its float64 run on every recorded
    tensor (`own_rounding` <= 1).  Gradients that vanish by cancellation through the first batch norm (a bias in front of it,
    the init embedding's bias) are pure rounding at about 1e-7 of the total gradient norm -- the floor of the rule -- and in
    about half of the seeds the reference's own rounding is beyond it (TSP-20 x 8, seeds 21 .. 69: between 0.51 and 2.8 times
    the bound, once 56): against such a recording even exact gradients fail.  Nothing of the code under test enters."""
    for data_seed in range(first_seed, first_seed + SEEDS_TRIED):
        ratio, where = _run_ppo_case(name, env_name, num_loc, batch, data_seed)
        if ratio <= 1.0:
            return
        print(f"{name}: data seed {data_seed} not used, the reference's own float32 rounding is {ratio:.2f} x the tolerance ({where})")
    raise RuntimeError(f"{name}: no data seed of {SEEDS_TRIED} qualifies")


def _run_ppo_case(name, env_name, num_loc, batch, data_seed, sample_seed=4321):
    Env = {"tsp": TSPEnv, "cvrp": CVRPEnv}[env_name]
    env = Env(generator_params=gen_params(env_name, num_loc), seed=data_seed)
    torch.manual_seed(data_seed)
    td = env.reset(batch_size=[batch])
    policy = make_policy(env_name).train()
    critic = create_critic_from_actor(policy)
    csd = critic.state_dict()
    for k, v in goldweights.fill_state_dict(csd).items():
        csd[k].copy_(torch.from_numpy(v))
    for k, v in policy.state_dict().items():          # the copied encoder IS the policy's (same key names, same streams)
        if k.startswith("encoder.") and v.is_floating_point():
            assert torch.equal(csd[k], v), k
    critic.train()

    # ppo.py:131-134
    torch.manual_seed(sample_seed)
    with torch.no_grad():
        out = policy(td.clone(), env, phase="train")
    actions, reward, ll_roll = out["actions"], out["reward"], out["log_likelihood"]
    ll_old = ll_roll + torch.tensor([PERTURB[i % len(PERTURB)] for i in range(batch)], dtype=ll_roll.dtype)

    # ppo.py:168-209 with sub_td = the whole batch.  Recorded from the float32 run, as the train fixtures are; the same lines are
    # also run in float64 on the same weights (the streams are exactly representable) to measure the rounding that is in the
    # recorded numbers (`own_rounding`)
    def mini_batch(dtype):
        pol, cri = copy.deepcopy(policy).to(dtype), copy.deepcopy(critic).to(dtype)
        sub_td = TensorDict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in td.items()}, batch_size=td.batch_size)
        previous_reward = reward.to(dtype).view(-1, 1)
        out = pol(sub_td.clone(), actions=actions, env=env, return_entropy=True, return_sum_log_likelihood=False)
        ll, entropy = out["log_likelihood"], out["entropy"]
        ratio = torch.exp(ll.sum(dim=-1) - ll_old.to(dtype)).view(-1, 1)
        value_pred = cri(sub_td)
        adv = previous_reward - value_pred.detach()
        unclipped, clipped = ratio * adv, torch.clamp(ratio, 1 - CLIP_RANGE, 1 + CLIP_RANGE) * adv
        surrogate_loss = -torch.min(unclipped, clipped).mean()
        value_loss = F.huber_loss(value_pred, previous_reward)
        loss = surrogate_loss + VF_LAMBDA * value_loss - ENTROPY_LAMBDA * entropy.mean()
        loss.backward()
        return dict(pol=pol, cri=cri, ll=ll, entropy=entropy, value=value_pred, ratio=ratio, took=(clipped < unclipped).view(-1),
                    loss=loss, surrogate_loss=surrogate_loss, value_loss=value_loss)

    r32, r = mini_batch(torch.float32), mini_batch(torch.float64)
    own = own_rounding(r32, r)
    if own[0] > 1.0:
        return own
    policy, critic = r32["pol"], r32["cri"]
    ll, entropy, value_pred, ratio, took_clipped = r32["ll"], r32["entropy"], r32["value"], r32["ratio"], r32["took"]
    loss, surrogate_loss, value_loss = r32["loss"], r32["surrogate_loss"], r32["value_loss"]
    assert bool(took_clipped.any()) and bool((~took_clipped).any()), "the fixture needs a clipped and an unclipped row"
    assert torch.equal(took_clipped, r["took"])

    fx = {
        "torch_version": np.array(torch.__version__), "env_name": np.array(env_name), "data_seed": np.array(data_seed),
        "own_rounding": np.array(own[0]),
        "clip_range": np.array(CLIP_RANGE), "vf_lambda": np.array(VF_LAMBDA), "entropy_lambda": np.array(ENTROPY_LAMBDA),
        "locs": np_(td["locs"]), "actions": np_(actions), "reward": np_(reward), "ll_rollout": np_(ll_roll), "ll_old": np_(ll_old),
        "ll": np_(ll), "entropy": np_(entropy), "value": np_(value_pred), "ratio": np_(ratio), "took_clipped": np_(took_clipped),
        "loss": np_(loss), "surrogate_loss": np_(surrogate_loss), "value_loss": np_(value_loss),
    }
    if env_name == "cvrp":
        fx["demand"] = np_(td["demand"])
    for tag, module in (("policy", policy), ("critic", critic)):
        names, norms = [], []
        for k, prm in module.named_parameters():
            g = prm.grad if prm.grad is not None else torch.zeros_like(prm)
            names.append(k)
            norms.append(float(g.double().norm()))
            if g.numel() <= 512:
                fx[f"{tag}_grad__{k}"] = np_(g)
        fx[f"{tag}_grad_names"] = np.array(names)
        fx[f"{tag}_grad_norms"] = np.array(norms, dtype=np.float64)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **fx)
    print(f"{name}: loss={float(loss):.6f} surrogate={float(surrogate_loss):.6f} value_loss={float(value_loss):.6f} "
          f"entropy={float(entropy.mean()):.6f} clipped rows={int(took_clipped.sum())}/{batch} "
          f"|grad policy|={np.sqrt((fx['policy_grad_norms'] ** 2).sum()):.6f} "
          f"|grad critic|={np.sqrt((fx['critic_grad_norms'] ** 2).sum()):.6f} -> {os.path.getsize(path) / 1024:.0f} KiB; "
          f"data seed {data_seed}; the reference's own float32 rounding: {own[0]:.2f} x the tolerance ({own[1]})")
    return own


def dump_critic_contract():
    """Key names / shapes / dtypes of the reference critic's state_dict (the checkpoint contract), as state_dict_contract.json."""
    import json

    out = {}
    for name, env_name in (("critic_am_tsp", "tsp"), ("critic_am_cvrp", "cvrp")):
        sd = create_critic_from_actor(make_policy(env_name)).state_dict()
        out[name] = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]
    with open(os.path.join(HERE, "state_dict_contract_critic.json"), "w") as f:
        json.dump(out, f, indent=0)
    print("state_dict_contract_critic.json:", {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    dump_critic_contract()
    run_ppo_case("ppo_tsp20", "tsp", 20, 8, first_seed=21)
    run_ppo_case("ppo_cvrp20", "cvrp", 20, 8, first_seed=22)
