#!/usr/bin/env python3
"""Generate the PolyNet golden vectors under tests/golden/ by RUNNING THE REFERENCE.

    python tests/golden/make_golden_polynet.py

Same machinery as make_golden.py / make_golden_ham.py (reference modules through `_refshim`, closed-form `goldweights`, recorded
Exp(1) noise, rollout fixtures whose data seeds are walked until `min_top2_gap >= 1e-4`).  The reference's
`zoo/polynet/__init__` imports the Lightning module and `zoo/polynet/policy.py` imports the MatNet encoder, so empty stub
packages are registered for `rl4co.models.zoo.polynet` and `rl4co.models.zoo.matnet` here, the way make_golden_ham.py does for
`zoo.ham`; the MatNet encoder is never constructed (encoder_type="AM").

PolyNet rolls out with `policy(td, env, num_starts=S, multisample=True)` (zoo/polynet/model.py:141-148): S rows per instance in
"(s b)" order, row s * B + b on strategy s % k.  In the reference's DecodingStrategy a `num_starts` above 1 switches multistart
on whatever `multisample` says (utils/decoding.py:249-255), so these rollouts begin with the forced start column of POMO (TSP:
node s % N, log-prob 0) and the decoder's first step already sees a first and a current node.  `how="num_samples"` records the
same rollout asked for as `num_samples=S`: no forced column, and TSP's first step uses the placeholder context.

Writes: state_dict_contract_polynet.json, the rollout fixtures polynet_*.npz (per-step selected log-probs, the encoder's
embeddings, the noise of the sampling ones) and train_polynet_tsp20.npz (PolyNet.calculate_loss with the shared baseline,
zoo/polynet/model.py:195-239, and every parameter's gradient).
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refshim  # noqa: E402,F401  (make_golden installs it)
import goldweights  # noqa: E402
from make_golden import Recorder, np_  # noqa: E402
from make_golden_pdp import MIN_GAP, SEEDS_TRIED, top2_gap  # noqa: E402

import torch  # noqa: E402

import rl4co.models.zoo.am.policy as ref_am_policy  # noqa: E402
from rl4co.envs.routing.cvrp.env import CVRPEnv  # noqa: E402
from rl4co.envs.routing.tsp.env import TSPEnv  # noqa: E402

_zoo = os.path.dirname(os.path.dirname(ref_am_policy.__file__))
for _name in ("polynet", "matnet"):
    if "rl4co.models.zoo." + _name not in sys.modules:
        _stub = types.ModuleType("rl4co.models.zoo." + _name)
        _stub.__path__ = [os.path.join(_zoo, _name)]
        sys.modules["rl4co.models.zoo." + _name] = _stub

from rl4co.models.zoo.polynet.policy import PolyNetPolicy  # noqa: E402

ENVS = {"tsp": TSPEnv, "cvrp": CVRPEnv}


def make_policy(env_name, k, **kw):
    pol = PolyNetPolicy(k=k, env_name=env_name, **kw).eval()
    sd = pol.state_dict()
    for key, v in goldweights.fill_state_dict(sd).items():
        if not key.endswith("binary_vectors"):            # the strategy table is part of the model, not a weight
            sd[key].copy_(torch.from_numpy(v))
    return pol


def _save(name, fx):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    assert size <= 1 << 20, f"{name}: {size} bytes is above the committed-file limit"
    return size


def contract():
    out = {}
    for env_name in ("tsp", "cvrp"):
        for k in (1, 2, 5, 8, 128):
            sd = PolyNetPolicy(k=k, env_name=env_name).state_dict()
            out[f"polynet_{env_name}_k{k}"] = [[key, list(v.shape), str(v.dtype).replace("torch.", "")] for key, v in sd.items()]
    with open(os.path.join(HERE, "state_dict_contract_polynet.json"), "w") as f:
        json.dump(out, f, indent=0)
    print("state_dict_contract_polynet.json:", {key: len(v) for key, v in out.items()})


def run_case(name, env_name, num_loc, batch, k, S, decode_type, first_seed, sample_seed=4321, actions=None, td_init=None,
             best_of=None, how="num_starts"):
    """best_of: a fixture with so many decisions that no seed reaches MIN_GAP (see main): the seed with the largest gap among
    `best_of` is recorded, and the gap it has is stored like any other."""
    policy = make_policy(env_name, k)
    sampling = decode_type == "sampling" and actions is None
    seeds = [first_seed + i for i in range(best_of or SEEDS_TRIED)] if td_init is None else [first_seed]
    best = None
    for data_seed in seeds:
        env = ENVS[env_name](generator_params=dict(num_loc=num_loc), seed=data_seed)
        if td_init is None:
            torch.manual_seed(data_seed)
            td0 = env.reset(batch_size=[batch])
        else:
            td0 = td_init
        torch.manual_seed(sample_seed)
        with torch.inference_mode(), Recorder(policy) as rec:
            out = policy(td0.clone(), env, phase="test", decode_type=decode_type, return_sum_log_likelihood=False,
                         return_hidden=True, actions=actions,
                         **(dict(num_starts=S, multisample=True) if how == "num_starts" else dict(num_samples=S)))
        gap = top2_gap(rec, sampling)
        if actions is not None or gap >= MIN_GAP:
            break
        if best_of:
            if best is None or gap > best[0]:
                best = (gap, data_seed, td0, out, rec)
            continue
        print(f"  {name}: seed {data_seed} has a top-2 gap of {gap:.3g} < {MIN_GAP}: next seed")
    else:
        if not best_of:
            raise SystemExit(f"{name}: none of the seeds {seeds[0]} .. {seeds[-1]} keeps the top-2 gap >= {MIN_GAP}")
        gap, data_seed, td0, out, rec = best
        print(f"  {name}: no seed of {seeds[0]} .. {seeds[-1]} reaches {MIN_GAP}; the largest top-2 gap, {gap:.3g}, is seed {data_seed}'s")
    fx = {
        "torch_version": np.array(torch.__version__), "env_name": np.array(env_name),
        "decode_type": np.array(decode_type if actions is None else "evaluate"),
        "k": np.array(k, dtype=np.int64), "num_starts": np.array(S, dtype=np.int64),
        "forced_start": np.array(how == "num_starts"),
        "data_seed": np.array(data_seed, dtype=np.int64), "min_top2_gap": np.array(gap, dtype=np.float64),
        "locs": np_(td0["locs"]), "actions": np_(out["actions"]), "reward": np_(out["reward"]),
        "logp_steps": np_(out["log_likelihood"]), "log_likelihood": np_(out["log_likelihood"].sum(1)),
        "embeddings": np_(out["hidden"].node_embeddings), "n_decoder_steps": np.array(len(rec.logits), dtype=np.int64),
    }
    if env_name == "cvrp":
        fx["demand"] = np_(td0["demand"])
    if rec.noise:
        fx["noise"] = np.stack([np_(q) for q in rec.noise], 1)      # [rows, T, M] Exp(1) draws
    size = _save(name, fx)
    print(f"{name}: seed={data_seed} T={len(rec.logits)} gap={gap:.3g} reward[:3]={fx['reward'][:3]} -> {size / 1024:.0f} KiB")
    return fx, td0


def train_case(name, num_loc, batch, k, data_seed=1234, sample_seed=4321):
    """PolyNet.shared_step in the train phase (zoo/polynet/model.py:124-158) on the policy in train() mode: a multisample
    sampling rollout with k solutions per instance, then calculate_loss with the shared baseline (baselines.py:57-61 gives
    reward.mean(dim=1, keepdims=True) and no baseline loss) -- the expressions of model.py:224-231, run here because the
    Lightning module itself cannot be imported."""
    from rl4co.utils.ops import unbatchify

    env = TSPEnv(generator_params=dict(num_loc=num_loc), seed=data_seed)
    torch.manual_seed(data_seed)
    td_init = env.reset(batch_size=[batch])
    policy = make_policy("tsp", k).train()
    torch.manual_seed(sample_seed)
    with Recorder(policy) as rec:
        out = policy(td_init.clone(), env, phase="train", num_starts=k, multisample=True, return_sum_log_likelihood=False,
                     return_hidden=True)
    logp = out["log_likelihood"]
    reward = unbatchify(out["reward"], (0, k))
    log_likelihood = unbatchify(logp.sum(1), (0, k))
    bl_val = reward.mean(dim=1, keepdims=True)
    best_idx = (-reward).argsort(1).argsort(1)
    mask = best_idx < 1
    advantage = reward - bl_val
    loss = -(advantage * log_likelihood * mask).mean()
    loss.backward()
    fx = {
        "torch_version": np.array(torch.__version__), "env_name": np.array("tsp"), "decode_type": np.array("sampling"),
        "k": np.array(k, dtype=np.int64), "num_starts": np.array(k, dtype=np.int64),
        "locs": np_(td_init["locs"]), "actions": np_(out["actions"]), "reward": np_(out["reward"]), "logp_steps": np_(logp),
        "loss": np_(loss), "noise": np.stack([np_(q) for q in rec.noise], 1),
        "embeddings": np_(out["hidden"].node_embeddings),
    }
    names, norms = [], []
    for key, prm in policy.named_parameters():
        if not prm.requires_grad:
            continue
        g = prm.grad if prm.grad is not None else torch.zeros_like(prm)
        names.append(key)
        norms.append(float(g.double().norm()))
        if g.numel() <= 512:
            fx["grad__" + key] = np_(g)
    fx["grad_names"] = np.array(names)
    fx["grad_norms"] = np.array(norms, dtype=np.float64)
    size = _save(name, fx)
    print(f"{name}: loss={float(loss.detach()):.6f} |grad|={np.sqrt((fx['grad_norms'] ** 2).sum()):.6f} -> {size / 1024:.0f} KiB")


def main():
    contract()
    run_case("polynet_tsp20_k5_s7_greedy", "tsp", 20, 3, 5, 7, "greedy", first_seed=3100)
    run_case("polynet_tsp20_k2_s17_greedy", "tsp", 20, 2, 2, 17, "greedy", first_seed=3200)
    run_case("polynet_tsp20_k1_s3_greedy", "tsp", 20, 2, 1, 3, "greedy", first_seed=3250)
    run_case("polynet_tsp20_k5_s7_samples_greedy", "tsp", 20, 3, 5, 7, "greedy", first_seed=3270, how="num_samples")
    fx, td0 = run_case("polynet_cvrp20_k8_s8_sampling", "cvrp", 20, 2, 8, 8, "sampling", first_seed=3300)
    run_case("polynet_cvrp20_k8_s8_evaluate", "cvrp", 20, 2, 8, 8, "sampling", first_seed=int(fx["data_seed"]),
             actions=torch.from_numpy(fx["actions"]), td_init=td0)
    # 2 x 128 rows x 100 steps = 25 600 greedy decisions.  Over 150 single instances (12 800 decisions each) the largest
    # smallest-gap was 3.0e-5 and the tenth largest 1.8e-5: the smallest gap of an instance falls off like exp(-1.5e5 gap), so a
    # batch of two reaches 1e-4 with a probability of about exp(-30).  No walk finds that; the best of 128 seeds is recorded.
    run_case("polynet_tsp100_k128_s128_greedy", "tsp", 100, 2, 128, 128, "greedy", first_seed=3400, best_of=128)
    run_case("polynet_tsp101_k16_s16_greedy", "tsp", 101, 1, 16, 16, "greedy", first_seed=3500)
    run_case("polynet_tsp112_k16_s16_greedy", "tsp", 112, 1, 16, 16, "greedy", first_seed=3600)
    train_case("train_polynet_tsp20", 20, 4, 4)


if __name__ == "__main__":
    main()
