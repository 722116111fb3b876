#!/usr/bin/env python3
"""Generate the Heterogeneous Attention Model (HAM) golden vectors under tests/golden/ by RUNNING THE REFERENCE.

    python tests/golden/make_golden_ham.py

Same machinery as make_golden.py / make_golden_pdp.py (reference modules through `_refshim`, closed-form `goldweights`, recorded
Exp(1) noise, rollout fixtures whose data seeds are walked until `min_top2_gap >= 1e-4`).  The reference's `zoo/ham/__init__`
imports the Lightning module, so an empty stub package is registered for `rl4co.models.zoo.ham` here, and
`AttentionModelPolicy` is set on the `rl4co.models.zoo.am` stub that `_refshim` registers (zoo/ham/policy.py imports it from
there).

Writes: state_dict_contract_ham.json, ham_mha_m{3,5,21,33}.npz, ham_embed_pdp20.npz, the rollout fixtures ham_pdp*.npz /
ham_pomo_pdp20_multistart_greedy.npz and train_ham_pdp20.npz.
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
import make_golden_pdp as mgp  # noqa: E402
from make_golden import Recorder, np_  # noqa: E402

import torch  # noqa: E402

import rl4co.models.zoo.am.policy as ref_am_policy  # noqa: E402
from rl4co.envs.routing.pdp.env import PDPEnv  # noqa: E402

sys.modules["rl4co.models.zoo.am"].AttentionModelPolicy = ref_am_policy.AttentionModelPolicy
if "rl4co.models.zoo.ham" not in sys.modules:
    _stub = types.ModuleType("rl4co.models.zoo.ham")
    _stub.__path__ = [os.path.join(os.path.dirname(os.path.dirname(ref_am_policy.__file__)), "ham")]
    sys.modules["rl4co.models.zoo.ham"] = _stub

from rl4co.models.zoo.ham.attention import HeterogenousMHA  # noqa: E402
from rl4co.models.zoo.ham.policy import HeterogeneousAttentionModelPolicy  # noqa: E402

POMO = mgp.POMO
WEIGHT_KEYS = ("W_query", "W_key", "W_val", "W1_query", "W2_query", "W3_query", "W4_query", "W5_query", "W6_query", "W_out")


def make_ham_policy(env_name="pdp", **kw):
    assert env_name == "pdp"
    pol = HeterogeneousAttentionModelPolicy(env_name=env_name, **kw).eval()
    sd = pol.state_dict()
    for k, v in goldweights.fill_state_dict(sd).items():
        sd[k].copy_(torch.from_numpy(v))
    return pol


def _save(name, fx):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    assert size <= 1 << 20, f"{name}: {size} bytes is above the committed-file limit"
    return size


def contract():
    out = {}
    for name, kw in {"am": dict(env_name="pdp"), "pomo": dict(env_name="pdp", **POMO)}.items():
        sd = HeterogeneousAttentionModelPolicy(**kw).state_dict()
        out[name] = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]
    with open(os.path.join(HERE, "state_dict_contract_ham.json"), "w") as f:
        json.dump(out, f, indent=0)
    print("state_dict_contract_ham.json:", {k: len(v) for k, v in out.items()})


def mha_case(M, B=2, E=128, H=8):
    """HeterogenousMHA.forward on randn inputs with the module's own init (seeded): float32 input and weights, the output of
    the module run in float64 (`out`) and in float32 (`out_float32`)."""
    torch.manual_seed(7000 + M)
    mod = HeterogenousMHA(H, E, E)
    x = torch.randn(B, M, E)
    with torch.no_grad():
        y32 = mod(x)
        y = mod.double()(x.double())            # the recorded output: the module itself in float64 on the float32 operands
        mod.float()
    fx = {"torch_version": np.array(torch.__version__), "x": np_(x), "out": np_(y), "out_float32": np_(y32)}
    for k in WEIGHT_KEYS:
        fx[k] = np_(getattr(mod, k))
    size = _save(f"ham_mha_m{M}", fx)
    print(f"ham_mha_m{M}: |out| <= {float(y.abs().max()):.3f} -> {size / 1024:.0f} KiB")


def embed_case(num_loc=20, batch=4, data_seed=1300):
    """Encoder embeddings (eval mode) of the batch-norm policy and of the instance-norm (POMO) policy on the same instances."""
    env = PDPEnv(generator_params=dict(num_loc=num_loc), seed=data_seed)
    torch.manual_seed(data_seed)
    td = env.reset(batch_size=[batch])
    fx = {"torch_version": np.array(torch.__version__), "locs": np_(td["locs"]), "data_seed": np.array(data_seed, dtype=np.int64)}
    for tag, kw in (("batch", {}), ("instance", POMO)):
        pol = make_ham_policy("pdp", **kw)
        with torch.inference_mode():
            h, init = pol.encoder(td)
        fx["embeddings_" + tag], fx["init_embeds_" + tag] = np_(h), np_(init)
    size = _save(f"ham_embed_pdp{num_loc}", fx)
    print(f"ham_embed_pdp{num_loc}: -> {size / 1024:.0f} KiB")


def train_case(name, num_loc, batch, data_seed=1234, sample_seed=4321):
    """make_golden.run_train_case for HAM on PDP (that function knows TSP / CVRP / SDVRP and the plain attention model only):
    one training forward + backward of the reference policy in train() mode with REINFORCE's loss without a baseline,
    loss = -(reward * log_likelihood).mean().  Same stored fields."""
    env = PDPEnv(generator_params=dict(num_loc=num_loc), seed=data_seed)
    torch.manual_seed(data_seed)
    td_init = env.reset(batch_size=[batch])
    policy = make_ham_policy("pdp").train()
    torch.manual_seed(sample_seed)
    with Recorder(policy) as rec:
        out = policy(td_init.clone(), env, phase="train", decode_type="sampling", return_sum_log_likelihood=False,
                     return_hidden=True)
    logp = out["log_likelihood"]
    ll, reward = logp.sum(1), out["reward"]
    loss = -(reward * ll).mean()
    loss.backward()
    fx = {
        "torch_version": np.array(torch.__version__), "env_name": np.array("pdp"), "decode_type": np.array("sampling"),
        "baseline": np.array("no"), "num_starts": np.array(0, dtype=np.int64),
        "locs": np_(td_init["locs"]), "actions": np_(out["actions"]), "reward": np_(reward), "logp_steps": np_(logp),
        "loss": np_(loss), "noise": np.stack([np_(q) for q in rec.noise], 1),
        "embeddings": np_(out["hidden"].node_embeddings),
    }
    names, norms = [], []
    for k, prm in policy.named_parameters():
        g = prm.grad if prm.grad is not None else torch.zeros_like(prm)
        names.append(k)
        norms.append(float(g.double().norm()))
        if g.numel() <= 512:
            fx["grad__" + k] = np_(g)
    fx["grad_names"] = np.array(names)
    fx["grad_norms"] = np.array(norms, dtype=np.float64)
    for k, b in policy.named_buffers():
        if k.endswith("running_mean") or k.endswith("running_var"):
            fx["buf__" + k] = np_(b)
    size = _save(name, fx)
    print(f"{name}: loss={float(loss.detach()):.6f} |grad|={np.sqrt((fx['grad_norms'] ** 2).sum()):.6f} -> {size / 1024:.0f} KiB")


def main():
    contract()
    for M in (3, 5, 21, 33):
        mha_case(M)
    embed_case()
    mgp.make_policy = make_ham_policy           # run_case builds its policy through this name
    mgp.run_case("ham_pdp4_greedy", 4, 4, "greedy", first_seed=2100)
    mgp.run_case("ham_pdp20_greedy", 20, 8, "greedy", first_seed=2200)
    mgp.run_case("ham_pdp20_sampling", 20, 8, "sampling", first_seed=2300)
    mgp.run_case("ham_pomo_pdp20_multistart_greedy", 20, 4, "multistart_greedy", policy_kw=POMO, num_starts=10, first_seed=2600)
    mgp.run_case("ham_pdp100_greedy", 100, 2, "greedy", first_seed=2700)
    mgp.run_case("ham_pdp128_greedy", 128, 2, "greedy", first_seed=2900)
    train_case("train_ham_pdp20", 20, 8)


if __name__ == "__main__":
    main()
