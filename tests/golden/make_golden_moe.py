#!/usr/bin/env python3
"""Generate the MoE-encoder (MVMoE) golden vectors under tests/golden/ by RUNNING THE REFERENCE.

    python tests/golden/make_golden_moe.py

Same machinery as make_golden.py / make_golden_pdp.py (reference modules through `_refshim`, closed-form `goldweights`, recorded
Exp(1) noise).  The policy is the reference's AttentionModelPolicy with moe_kwargs = {"encoder": MOE, "decoder": None}: every
encoder layer's feed-forward sublayer is the sparsely gated mixture of experts of rl4co/models/nn/moe.py.

NEAR TIES ARE EXCLUDED HERE, NOT IN THE TESTS.  Besides `min_top2_gap` (make_golden_pdp.py: the smallest gap between the best and
the second-best feasible log-prob over every row and step) every rollout fixture stores `min_gate_gap`: the smallest difference
between the k-th and the (k+1)-th largest gate probability over all layers and rows.  The script walks the data seeds (32 at
most, then it fails) until both are at least MIN_GAP = 1e-4, ten times the 1e-5 agreement held between the restatement and the
reference, so that no routing decision and no tour in a fixture can flip inside that agreement.

The 6-layer instance-norm (POMO) policy does not meet the gate condition with the closed-form `w_gate` (its deep layers'
softmax saturates: the k-th and (k+1)-th probabilities are both next to zero).  Its fixture therefore carries its own `w_gate`
arrays, as data: the closed-form ones times `w_gate_scale`, the first of 1, 1/2, 1/4, ... for which a seed qualifies.

The training-mode fixture (batch statistics) is in the same position and is treated the same way.

Writes: state_dict_contract_moe.json, the rollout fixtures moe_*.npz, moe_module_train.npz (one MoE module in training mode with
its recorded standard-normal draw) and train_moe_cvrp20.npz (one REINFORCE step's gradients, noisy_gating off).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refshim  # noqa: E402,F401  (make_golden installs it)
import goldweights  # noqa: E402
from make_golden import Recorder, make_policy, np_  # noqa: E402
from make_golden_pdp import top2_gap  # noqa: E402

import torch  # noqa: E402

from rl4co.envs.routing.cvrp.env import CVRPEnv  # noqa: E402
from rl4co.envs.routing.tsp.env import TSPEnv  # noqa: E402
from rl4co.models.nn.moe import MoE  # noqa: E402
from rl4co.models.zoo.am.policy import AttentionModelPolicy  # noqa: E402

MIN_GAP = 1e-4
SEEDS_TRIED = 32
MOE = dict(hidden_act="ReLU", num_experts=4, k=2, noisy_gating=True)
POMO = dict(num_encoder_layers=6, normalization="instance", use_graph_context=False)
ENVS = {"tsp": TSPEnv, "cvrp": CVRPEnv}


def moe_kwargs(**over):
    return {"encoder": dict(MOE, **over), "decoder": None}


class GateRecorder:
    """Per encoder layer: the gate probabilities softmax(x w_gate) of every row, the reference's top-k choice and the layer's
    output embeddings."""

    def __init__(self, policy):
        self.layers = list(policy.encoder.net.layers)
        self.probs, self.sel, self.emb, self._undo = [], [], [], []

    def __enter__(self):
        for layer in self.layers:
            moe = layer[2].module
            orig = moe.noisy_top_k_gating

            def gating(x, train, noise_epsilon=1e-2, _moe=moe, _orig=orig):
                gates, load = _orig(x, train, noise_epsilon)
                if not (train and _moe.noisy_gating):
                    p = _moe.softmax(x @ _moe.w_gate)
                    self.probs.append(p.detach().clone())
                    self.sel.append(p.topk(_moe.k, dim=-1).indices.detach().clone())
                return gates, load

            moe.noisy_top_k_gating = gating
            self._undo.append((moe, orig))
            self._undo.append(layer.register_forward_hook(lambda m, i, o: self.emb.append(o.detach().clone())))
        return self

    def __exit__(self, *exc):
        for u in self._undo:
            if isinstance(u, tuple):
                u[0].noisy_top_k_gating = u[1]
            else:
                u.remove()

    def min_gap(self, k):
        gap = np.inf
        for p in self.probs:
            if k < p.shape[-1]:
                s = p.double().sort(-1, descending=True).values
                gap = min(gap, float((s[:, k - 1] - s[:, k]).min()))
        return gap


def scaled_policy(env_name, policy_kw, scale):
    policy = make_policy(env_name, moe_kwargs=moe_kwargs(), **policy_kw)
    if scale != 1.0:
        with torch.no_grad():
            for layer in policy.encoder.net.layers:
                layer[2].module.w_gate.mul_(scale)
    return policy


def run_case(name, env_name, num_loc, batch, decode_type, policy_kw=None, num_starts=None, first_seed=1, sample_seed=4321,
             actions=None, td_init=None, scale=1.0, may_fail=False):
    policy_kw = policy_kw or {}
    policy = scaled_policy(env_name, policy_kw, scale)
    k = MOE["k"]
    kw = dict(decode_type=decode_type)
    if num_starts is not None:
        kw["num_starts"] = num_starts
    sampling = "sampling" in decode_type and actions is None
    seeds = [first_seed + i for i in range(SEEDS_TRIED)] if td_init is None else [first_seed]
    for data_seed in seeds:
        env = ENVS[env_name](generator_params=dict(num_loc=num_loc), seed=data_seed)
        if td_init is None:
            torch.manual_seed(data_seed)
            td0 = env.reset(batch_size=[batch])
        else:
            td0 = td_init
        torch.manual_seed(sample_seed)
        with torch.inference_mode(), Recorder(policy) as rec, GateRecorder(policy) as gr:
            out = policy(td0.clone(), env, phase="test", return_sum_log_likelihood=False, actions=actions, **kw)
        gap, ggap = top2_gap(rec, sampling), gr.min_gap(k)
        if (actions is not None or gap >= MIN_GAP) and ggap >= MIN_GAP:
            break
        print(f"  {name}: seed {data_seed}: top-2 gap {gap:.3g}, gate gap {ggap:.3g} (need {MIN_GAP}): next seed")
    else:
        if may_fail:
            return None, None
        raise SystemExit(f"{name}: none of the seeds {seeds[0]} .. {seeds[-1]} keeps both gaps >= {MIN_GAP}")
    T = len(rec.logits)
    fx = {
        "torch_version": np.array(torch.__version__),
        "env_name": np.array(env_name),
        "decode_type": np.array(decode_type if actions is None else "evaluate"),
        "num_starts": np.array(0 if num_starts is None else num_starts, dtype=np.int64),
        "data_seed": np.array(data_seed, dtype=np.int64),
        "min_top2_gap": np.array(gap, dtype=np.float64),
        "min_gate_gap": np.array(ggap, dtype=np.float64),
        "num_experts": np.array(MOE["num_experts"], dtype=np.int64),
        "k": np.array(k, dtype=np.int64),
        "w_gate_scale": np.array(scale, dtype=np.float64),
        "locs": np_(td0["locs"]),
        "actions": np_(out["actions"]),
        "reward": np_(out["reward"]),
        "logp_steps": np_(out["log_likelihood"]),
        "log_likelihood": np_(out["log_likelihood"].sum(1)),
        "n_decoder_steps": np.array(T, dtype=np.int64),
        "layer_embeddings": np.stack([np_(e) for e in gr.emb]),                       # [layers, B, M, E]
        "gate_probs": np.stack([np_(p) for p in gr.probs]),                            # [layers, B * M, num_experts]
        "gate_sel": np.stack([np_(s) for s in gr.sel]).astype(np.int8),                # [layers, B * M, k], larger first
    }
    if env_name == "cvrp":
        fx["demand"] = np_(td0["demand"])
        fx["vehicle_capacity"] = np_(td0["vehicle_capacity"])
    if rec.noise:
        fx["noise"] = np.stack([np_(q) for q in rec.noise], 1)                         # [rows, T, M] Exp(1) draws
    for kk, v in policy_kw.items():
        fx["policy_kw_" + kk] = np.array(v)
    if scale != 1.0:
        for li, layer in enumerate(policy.encoder.net.layers):
            fx[f"w_gate_{li}"] = np_(layer[2].module.w_gate)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    assert size <= 1 << 20, f"{name}: {size} bytes is above the committed-file limit"
    print(f"{name}: seed={data_seed} scale={scale} T={T} top-2 gap={gap:.3g} gate gap={ggap:.3g} "
          f"reward[:3]={fx['reward'][:3]} -> {size / 1024:.0f} KiB")
    return fx, td0


def pomo_case(name, num_loc, batch, num_starts, first_seed):
    scale = 1.0
    while scale >= 1.0 / 1024:
        fx, td0 = run_case(name, "cvrp", num_loc, batch, "multistart_greedy", policy_kw=POMO, num_starts=num_starts,
                           first_seed=first_seed, scale=scale, may_fail=True)
        if fx is not None:
            return fx, td0
        print(f"  {name}: no seed qualifies with w_gate scaled by {scale}: halving")
        scale /= 2
    raise SystemExit(f"{name}: no w_gate scale down to 1/1024 qualifies")


def module_train_case(name="moe_module_train", rows=37, seed=11):
    """One MoE module in training mode: its input, the recorded torch.randn_like draw, the gates and the output."""
    moe = MoE(128, 128, num_neurons=[512], **MOE).train()
    sd = moe.state_dict()
    pre = "encoder.net.layers.0.2.module."
    for kk, v in sd.items():
        w = goldweights.tensor_for(pre + kk, tuple(v.shape))
        if w is not None:
            v.copy_(torch.from_numpy(w))
    x = torch.from_numpy(goldweights.unit(name + ".x", rows * 128).reshape(rows, 128))
    drawn = []
    orig = torch.randn_like

    def randn_like(t, *a, **kw):
        n = orig(t, *a, **kw)
        drawn.append(n.clone())
        return n

    torch.manual_seed(seed)
    torch.randn_like = randn_like
    try:
        with torch.no_grad():
            gates, _ = moe.noisy_top_k_gating(x, True)
            torch.manual_seed(seed)
            del drawn[:]
            y = moe(x)
    finally:
        torch.randn_like = orig
    assert len(drawn) == 1
    with torch.no_grad():
        noisy = x @ moe.w_gate + drawn[0] * (torch.nn.functional.softplus(x @ moe.w_noise) + 1e-2)
        p = torch.softmax(noisy, -1)
    s = p.double().sort(-1, descending=True).values
    ggap = float((s[:, MOE["k"] - 1] - s[:, MOE["k"]]).min())
    assert ggap >= MIN_GAP, f"{name}: gate gap {ggap:.3g}; choose another seed"
    fx = {"torch_version": np.array(torch.__version__), "x": np_(x), "randn": np_(drawn[0]), "gates": np_(gates), "y": np_(y),
          "gate_probs": np_(p), "gate_sel": np_(p.topk(MOE["k"], dim=-1).indices).astype(np.int8),
          "min_gate_gap": np.array(ggap), "num_experts": np.array(MOE["num_experts"], dtype=np.int64),
          "k": np.array(MOE["k"], dtype=np.int64), "key_prefix": np.array(pre)}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **fx)
    print(f"{name}: rows={rows} gate gap={ggap:.3g}")


def train_case(name="train_moe_cvrp20", num_loc=20, batch=8, first_seed=1, sample_seed=4321):
    """One REINFORCE step (no baseline) of the reference policy in train() mode with noisy_gating off: sampled tours with their
    recorded noise, loss, every parameter's gradient (norm; full tensors for the small ones), batch-norm running statistics."""
    k = MOE["k"]
    for scale, data_seed in ((2.0 ** -i, first_seed + j) for i in range(11) for j in range(SEEDS_TRIED)):
        policy = make_policy("cvrp", moe_kwargs=moe_kwargs(noisy_gating=False)).train()
        with torch.no_grad():
            for layer in policy.encoder.net.layers:
                layer[2].module.w_gate.mul_(scale)
        env = CVRPEnv(generator_params=dict(num_loc=num_loc), seed=data_seed)
        torch.manual_seed(data_seed)
        td0 = env.reset(batch_size=[batch])
        torch.manual_seed(sample_seed)
        with Recorder(policy) as rec, GateRecorder(policy) as gr:
            out = policy(td0.clone(), env, phase="train", decode_type="sampling", return_sum_log_likelihood=False)
        gap, ggap = top2_gap(rec, True), gr.min_gap(k)
        if gap >= MIN_GAP and ggap >= MIN_GAP:
            break
        if data_seed == first_seed + SEEDS_TRIED - 1:
            print(f"  {name}: no seed qualifies with w_gate scaled by {scale} (last: top-2 gap {gap:.3g}, gate gap {ggap:.3g})")
    else:
        raise SystemExit(f"{name}: no w_gate scale down to 1/1024 qualifies")
    logp = out["log_likelihood"]
    ll, reward = logp.sum(1), out["reward"]
    loss = -(reward * ll).mean()
    loss.backward()
    fx = {"torch_version": np.array(torch.__version__), "env_name": np.array("cvrp"), "data_seed": np.array(data_seed),
          "min_top2_gap": np.array(gap), "min_gate_gap": np.array(ggap), "locs": np_(td0["locs"]), "demand": np_(td0["demand"]),
          "vehicle_capacity": np_(td0["vehicle_capacity"]), "actions": np_(out["actions"]), "reward": np_(reward),
          "logp_steps": np_(logp), "loss": np_(loss), "noise": np.stack([np_(q) for q in rec.noise], 1),
          "gate_sel": np.stack([np_(s) for s in gr.sel]).astype(np.int8), "w_gate_scale": np.array(scale)}
    for li, layer in enumerate(policy.encoder.net.layers):      # as data, like the POMO fixture's (batch statistics saturate
        fx[f"w_gate_{li}"] = np_(layer[2].module.w_gate)        # the closed-form gate)
    names, norms = [], []
    for kk, prm in policy.named_parameters():
        g = prm.grad if prm.grad is not None else torch.zeros_like(prm)
        names.append(kk)
        norms.append(float(g.double().norm()))
        if g.numel() <= 512:
            fx["grad__" + kk] = np_(g)
    fx["grad_names"] = np.array(names)
    fx["grad_norms"] = np.array(norms, dtype=np.float64)
    for kk, b in policy.named_buffers():
        if kk.endswith("running_mean") or kk.endswith("running_var"):
            fx["buf__" + kk] = np_(b)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **fx)
    print(f"{name}: seed={data_seed} scale={scale} loss={float(loss):.6f} |grad|={np.sqrt((fx['grad_norms'] ** 2).sum()):.6f} "
          f"gate gap={ggap:.3g} -> {os.path.getsize(path) / 1024:.0f} KiB")


def contract():
    out = {}
    for name, kw in {"am_cvrp_moe": dict(env_name="cvrp"), "pomo_cvrp_moe": dict(env_name="cvrp", **POMO),
                     "am_tsp_moe": dict(env_name="tsp")}.items():
        sd = AttentionModelPolicy(moe_kwargs=moe_kwargs(), **kw).state_dict()
        out[name] = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]
    with open(os.path.join(HERE, "state_dict_contract_moe.json"), "w") as f:
        json.dump(out, f, indent=0)
    print("state_dict_contract_moe.json:", {k: len(v) for k, v in out.items()})
    # documented difference: with the zero-initialised w_gate every row ties, and torch.topk's tie order is its own
    print("torch.topk of four equal values:", torch.full((1, 4), 0.25).topk(3, dim=-1).indices.tolist())


def main():
    contract()
    run_case("moe_tsp20_greedy", "tsp", 20, 8, "greedy", first_seed=1)
    run_case("moe_cvrp20_greedy", "cvrp", 20, 8, "greedy", first_seed=1)
    fx, td0 = run_case("moe_cvrp20_sampling", "cvrp", 20, 8, "sampling", first_seed=1)
    run_case("moe_cvrp20_evaluate", "cvrp", 20, 8, "sampling", actions=torch.from_numpy(fx["actions"]), td_init=td0,
             first_seed=int(fx["data_seed"]))
    pomo_case("moe_pomo_cvrp20_multistart_greedy", 20, 4, 10, first_seed=1)
    run_case("moe_cvrp112_greedy", "cvrp", 112, 2, "greedy", first_seed=1)
    module_train_case()
    train_case()


if __name__ == "__main__":
    main()
