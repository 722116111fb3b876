#!/usr/bin/env python3
"""Generate the Pointer Network golden vectors under tests/golden/ by RUNNING THE REFERENCE.

    python tests/golden/make_golden_ptrnet.py

The reference's zoo/ptrnet/{policy,encoder,decoder}.py run unmodified through `_refshim`; an empty package module stands for
`rl4co.models.zoo.ptrnet`, whose `__init__` imports the Lightning module.  Weights are closed-form (tests/ptrnet_ref.py,
`closed_form_weights`): the default initialisation gives near-uniform distributions with exact greedy ties.  Per-step log-probs
come from wrapping `decode_logprobs` as the decoder imported it, the Exp(1) draws from replaying `torch.multinomial` the way
`make_golden.Recorder` does.

Every fixture also holds the reference's float64 run on the same tours (`policy.double()`, inputs `.double()`, float64 as the
default dtype around the call, the tours given as `eval_tours`): `logp64`, `err32 = max |logp32 - logp64|` and `min_top2_gap`.
A fixture is kept only if min_top2_gap >= 1e-4 >= 20 * err32; at most 32 data seeds are walked, and the script fails otherwise.
(Greedy fixtures of 100 nodes and more do not qualify within 32 seeds and are not asked for.)

Writes state_dict_contract_ptrnet.json, ptrnet{5,20}_greedy, ptrnet{2,20,100,113,128}_sampling, ptrnet20_evaluate and
train_ptrnet_tsp20 (.npz)."""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _refshim  # noqa: E402

_refshim.install()

import torch  # noqa: E402

import rl4co.models.zoo.am.policy as ref_am_policy  # noqa: E402
from rl4co.envs.routing.tsp.env import TSPEnv  # noqa: E402

_zoo = os.path.dirname(os.path.dirname(ref_am_policy.__file__))
if "rl4co.models.zoo.ptrnet" not in sys.modules:
    _stub = types.ModuleType("rl4co.models.zoo.ptrnet")
    _stub.__path__ = [os.path.join(_zoo, "ptrnet")]
    sys.modules["rl4co.models.zoo.ptrnet"] = _stub

import rl4co.models.zoo.ptrnet.decoder as ref_decoder  # noqa: E402
from rl4co.models.zoo.ptrnet.policy import PointerNetworkPolicy  # noqa: E402

from ptrnet_ref import closed_form_weights  # noqa: E402

MIN_GAP = 1e-4
SEEDS_TRIED = 32


def np_(t):
    return t.detach().cpu().numpy()


def make_policy():
    pol = PointerNetworkPolicy()
    sd = pol.state_dict()
    for key, v in closed_form_weights({k: tuple(v.shape) for k, v in sd.items()}).items():
        sd[key].copy_(v)
    return pol


class Recorder:
    """Per-step log-probs [B, N] (what the decoder hands to decode_logprobs), the policy's chosen-node log-probs [B, N] (the
    first result of `_inner`) and the Exp(1) draws of torch.multinomial."""

    def __init__(self, policy):
        self.policy = policy
        self.logprobs, self.noise, self.selected = [], [], None

    def __enter__(self):
        self._dl = ref_decoder.decode_logprobs

        def dl(logprobs, mask, decode_type="sampling"):
            self.logprobs.append(logprobs.detach().clone())
            return self._dl(logprobs, mask, decode_type=decode_type)

        ref_decoder.decode_logprobs = dl
        self._inner = self.policy._inner

        def inner(*a, **k):
            lp, idx = self._inner(*a, **k)
            self.selected = lp.detach().clone()
            return lp, idx

        self.policy._inner = inner
        self._mn = torch.multinomial

        def mn(probs, num_samples, *a, **k):
            state = torch.get_rng_state()
            res = self._mn(probs, num_samples, *a, **k)
            after = torch.get_rng_state()
            torch.set_rng_state(state)
            q = torch.empty_like(probs).exponential_(1)
            assert torch.equal(torch.argmax(probs / q, dim=-1, keepdim=True), res), "multinomial != argmax(p / Exp(1)) replay"
            torch.set_rng_state(after)
            self.noise.append(q.clone())
            return res

        torch.multinomial = mn
        return self

    def __exit__(self, *exc):
        ref_decoder.decode_logprobs = self._dl
        del self.policy._inner
        torch.multinomial = self._mn


def top2_gap(rec, sampling):
    gap = np.inf
    for t, lp in enumerate(rec.logprobs):
        key = lp.double()
        if sampling:
            key = key - rec.noise[t].double().log()
        top = torch.topk(key, 2, dim=-1).values
        d = top[:, 0] - top[:, 1]
        d = d[torch.isfinite(d)]
        if d.numel():
            gap = min(gap, float(d.min()))
    return gap


def run64(locs, tours):
    """The reference in float64 on given tours: chosen-node log-probs [B, N]."""
    env = TSPEnv(generator_params=dict(num_loc=locs.shape[1]))
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        pol = make_policy().double().eval()
        td = env.reset(_refshim.TensorDict({"locs": locs.double()}, batch_size=[locs.shape[0]]))
        with torch.inference_mode(), Recorder(pol) as rec:
            pol(td, env, phase="test", decode_type="greedy", eval_tours=tours)
    finally:
        torch.set_default_dtype(prev)
    assert rec.selected.dtype == torch.float64
    return rec.selected


def _save(name, fx):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    assert size <= 1 << 20, f"{name}: {size} bytes is above the committed-file limit"
    return size


def contract():
    sd = PointerNetworkPolicy().state_dict()
    out = {"ptrnet_tsp": [[key, list(v.shape), str(v.dtype).replace("torch.", "")] for key, v in sd.items()]}
    with open(os.path.join(HERE, "state_dict_contract_ptrnet.json"), "w") as f:
        json.dump(out, f, indent=0)
    print("state_dict_contract_ptrnet.json:", len(out["ptrnet_tsp"]), "entries")


def run_case(name, num_loc, batch, decode_type, first_seed, sample_seed=4321, tours=None, locs=None):
    policy = make_policy().eval()
    sampling = decode_type == "sampling" and tours is None
    seeds = [first_seed + i for i in range(SEEDS_TRIED)] if locs is None else [first_seed]
    for data_seed in seeds:
        env = TSPEnv(generator_params=dict(num_loc=num_loc), seed=data_seed)
        if locs is None:
            torch.manual_seed(data_seed)
            td0 = env.reset(batch_size=[batch])
        else:
            td0 = env.reset(_refshim.TensorDict({"locs": locs}, batch_size=[batch]))
        torch.manual_seed(sample_seed)
        with torch.inference_mode(), Recorder(policy) as rec:
            out = policy(td0.clone(), env, phase="test", decode_type=decode_type, eval_tours=tours)
        logp32 = rec.selected
        logp64 = run64(td0["locs"], out["actions"])
        err32 = float((logp32.double() - logp64).abs().max())
        gap = top2_gap(rec, sampling) if tours is None else float("inf")
        if gap >= MIN_GAP and MIN_GAP >= 20 * err32:
            break
        print(f"  {name}: seed {data_seed}: top-2 gap {gap:.3g}, err32 {err32:.3g}: next seed")
    else:
        raise SystemExit(f"{name}: none of the seeds {seeds[0]} .. {seeds[-1]} has min_top2_gap >= {MIN_GAP} >= 20 err32")
    fx = {
        "torch_version": np.array(torch.__version__), "env_name": np.array("tsp"),
        "decode_type": np.array(decode_type if tours is None else "evaluate"),
        "data_seed": np.array(data_seed, dtype=np.int64), "min_top2_gap": np.array(gap, dtype=np.float64),
        "err32": np.array(err32, dtype=np.float64),
        "locs": np_(td0["locs"]), "actions": np_(out["actions"]), "reward": np_(out["reward"]),
        "logp_steps": np_(logp32), "logp64": np_(logp64), "log_likelihood": np_(out["log_likelihood"]),
    }
    if rec.noise:
        fx["noise"] = np.stack([np_(q) for q in rec.noise], 1)      # [B, N steps, N nodes] Exp(1) draws
    size = _save(name, fx)
    print(f"{name}: seed={data_seed} gap={gap:.3g} err32={err32:.3g} reward[:2]={fx['reward'][:2]} -> {size / 1024:.0f} KiB")
    return fx, td0


def train_case(name, num_loc, batch, data_seed=1234, sample_seed=4321):
    """One train-phase step: a sampled rollout under autograd, loss = -((R - mean R) * ll).mean() (REINFORCE with the batch-mean
    baseline, reinforce.py:103-106), backward.  Stored: the draws, the loss, every parameter's gradient norm (the two unused
    encoder parameters get none: 0) and the full gradients of the decoder's attentions."""
    env = TSPEnv(generator_params=dict(num_loc=num_loc), seed=data_seed)
    torch.manual_seed(data_seed)
    td0 = env.reset(batch_size=[batch])
    policy = make_policy().train()
    torch.manual_seed(sample_seed)
    with Recorder(policy) as rec:
        out = policy(td0.clone(), env, phase="train", decode_type="sampling")
    reward, ll = out["reward"], out["log_likelihood"]
    loss = -((reward - reward.mean()) * ll).mean()
    loss.backward()
    fx = {
        "torch_version": np.array(torch.__version__), "env_name": np.array("tsp"), "decode_type": np.array("sampling"),
        "locs": np_(td0["locs"]), "actions": np_(out["actions"]), "reward": np_(reward), "logp_steps": np_(rec.selected),
        "log_likelihood": np_(ll), "loss": np_(loss), "noise": np.stack([np_(q) for q in rec.noise], 1),
        "min_top2_gap": np.array(top2_gap(rec, True), dtype=np.float64),
    }
    names, norms, has = [], [], []
    for key, prm in policy.named_parameters():
        g = prm.grad if prm.grad is not None else torch.zeros_like(prm)
        names.append(key)
        norms.append(float(g.double().norm()))
        has.append(prm.grad is not None)
        if key.startswith("decoder.pointer.") or key.startswith("decoder.glimpse."):
            fx["grad__" + key] = np_(g)
    fx["grad_names"] = np.array(names)
    fx["grad_norms"] = np.array(norms, dtype=np.float64)
    fx["grad_present"] = np.array(has)
    size = _save(name, fx)
    print(f"{name}: loss={float(loss.detach()):.6f} |grad|={np.sqrt((fx['grad_norms'] ** 2).sum()):.6f} "
          f"gap={float(fx['min_top2_gap']):.3g} -> {size / 1024:.0f} KiB")


def main():
    contract()
    run_case("ptrnet5_greedy", 5, 4, "greedy", first_seed=5100)
    run_case("ptrnet20_greedy", 20, 4, "greedy", first_seed=5200)
    run_case("ptrnet2_sampling", 2, 4, "sampling", first_seed=5300)
    fx, td0 = run_case("ptrnet20_sampling", 20, 4, "sampling", first_seed=5400)
    run_case("ptrnet20_evaluate", 20, 4, "sampling", first_seed=int(fx["data_seed"]), tours=torch.from_numpy(fx["actions"]),
             locs=td0["locs"])
    run_case("ptrnet100_sampling", 100, 2, "sampling", first_seed=5500)
    run_case("ptrnet113_sampling", 113, 2, "sampling", first_seed=5600)
    run_case("ptrnet128_sampling", 128, 2, "sampling", first_seed=5700)
    train_case("train_ptrnet_tsp20", 20, 4)


if __name__ == "__main__":
    main()
