"""The yardstick of the MoE-encoder (MVMoE) tests: the defined arithmetic of the mixture-of-experts feed-forward sublayer
(include/eamrl.h, eamrl_moe_ffn; DESIGN.md "MoE encoder"), built from the CPU oracle as it stands.

Per row x (a node embedding after the attention sublayer's norm), everything float32, one rounding per written operation:

  gate logit   logit[e] = oracle.linear(x, w_gate^T)            the k-ordered fma chain from 0
  noise        std[e] = softplus(oracle.linear(x, w_noise^T)) + float32(1e-2), softplus(v) = v > 20 ? v : log(1 + exp(v)) on
               oracle.math_fn("exp" / "log");  logit[e] = logit[e] + noise[e] * std[e]  (multiply, then add)
  softmax      exp(logit - max) through oracle.math_fn("exp"), summed in ascending expert order, one division per expert
  selection    the k largest p, larger first, TIES TO THE LOWER EXPERT INDEX (torch.topk's tie order is its own: for four equal
               values the reference picks [2, 3]; trained gates do not tie)
  gates        g[j] = p[sel j] / (sum_j p[sel j] + float32(1e-6)), the sum in selection order
  experts      o_e = oracle.linear(oracle.linear(x, W1_e, b1_e, relu), W2_e, b2_e)
  combine      y = 0, then for the selected experts in ASCENDING expert index  y = y + g_e * o_e  (multiply, then add; an
               expert that is not selected is skipped)
  finish       h + y, then the layer's second Normalization as oracle.encode applies it

The rest of the model is the oracle's: `encode` is the layer loop of oracle.encode with this sublayer in place of the MLP,
`policy_rollout` is oracle.policy_rollout around it.  tests/test_host_moe.py pins this module to the reference's recorded
results; tests/test_gpu_moe.py holds the HIP kernels to it bit for bit.  Results per fixture are computed once (`reference`).
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import goldweights
from _util import GOLDEN, golden
from oracle import oracle as orc

ROLLOUT_FIXTURES = ["moe_tsp20_greedy", "moe_cvrp20_greedy", "moe_cvrp20_sampling", "moe_cvrp20_evaluate",
                    "moe_pomo_cvrp20_multistart_greedy", "moe_cvrp112_greedy"]
MOE_KWARGS = {"encoder": {"hidden_act": "ReLU", "num_experts": 4, "k": 2, "noisy_gating": True}, "decoder": None}

with open(os.path.join(GOLDEN, "state_dict_contract_moe.json")) as _f:
    CONTRACT = json.load(_f)

f32 = np.float32


def cfg_for(fx):
    return ("pomo_" if "policy_kw_num_encoder_layers" in fx else "am_") + str(fx["env_name"]) + "_moe"


def weights(cfg, fx=None):
    """{key: float32 ndarray} of the closed-form weights for a contract config; a fixture's own `w_gate_<layer>` arrays (the
    gate scaled when the fixture was made) replace the closed-form gate."""
    sd = {}
    for k, shape, dt in CONTRACT[cfg]:
        if dt == "float32":
            v = goldweights.tensor_for(k, shape)
            if v is not None:
                sd[k] = v
    layer = 0
    while fx is not None and f"w_gate_{layer}" in fx:
        sd[f"encoder.net.layers.{layer}.2.module.w_gate"] = np.ascontiguousarray(fx[f"w_gate_{layer}"], f32)
        layer += 1
    return sd


def _fn(name, x):
    x = np.ascontiguousarray(x, f32)
    return orc.math_fn(name, x.view(np.uint32)).view(f32).reshape(x.shape)


def softplus(v):
    v = np.ascontiguousarray(v, f32)
    soft = _fn("log", f32(1.0) + _fn("exp", v))
    return np.where(v > f32(20.0), v, soft).astype(f32)


def gate(x, w_gate, k, w_noise=None, noise=None):
    """x [rows, E], w_gate / w_noise [E, n_exp], noise [rows, n_exp] or None -> (p [rows, n_exp], sel [rows, k] int8, larger
    first, g [rows, k])."""
    x = np.ascontiguousarray(x, f32)
    logit = orc.linear(x, np.ascontiguousarray(np.asarray(w_gate, f32).T))
    if noise is not None:
        std = softplus(orc.linear(x, np.ascontiguousarray(np.asarray(w_noise, f32).T))) + f32(1e-2)
        nz = (np.ascontiguousarray(noise, f32) * std).astype(f32)
        logit = (logit + nz).astype(f32)
    rows, n = logit.shape
    mx = logit.max(-1, keepdims=True)
    ex = _fn("exp", (logit - mx).astype(f32))
    tot = np.zeros(rows, f32)
    for e in range(n):
        tot = (tot + ex[:, e]).astype(f32)
    p = (ex / tot[:, None]).astype(f32)
    sel = np.zeros((rows, k), np.int8)
    sp = np.zeros((rows, k), f32)
    taken = np.zeros((rows, n), bool)
    r = np.arange(rows)
    for j in range(k):
        best = np.full(rows, -1, np.int64)
        bv = np.zeros(rows, f32)
        for e in range(n):
            better = ~taken[:, e] & ((best < 0) | (p[:, e] > bv))          # strict: ties stay with the lower index
            best = np.where(better, e, best)
            bv = np.where(better, p[:, e], bv).astype(f32)
        taken[r, best] = True
        sel[:, j] = best
        sp[:, j] = bv
    s = np.zeros(rows, f32)
    for j in range(k):
        s = (s + sp[:, j]).astype(f32)
    s = (s + f32(1e-6)).astype(f32)
    return p, sel, (sp / s[:, None]).astype(f32)


def experts_of(sd, prefix):
    """[(W1, b1, W2, b2)] of the MoE module whose keys start with `prefix` (".../2.module.")."""
    out = []
    while f"{prefix}experts.{len(out)}.lins.0.weight" in sd:
        q = f"{prefix}experts.{len(out)}.lins."
        out.append(tuple(np.ascontiguousarray(sd[q + s], f32) for s in ("0.weight", "0.bias", "1.weight", "1.bias")))
    return out


def combine(x, experts, sel, g):
    """y [rows, E]: for every row its selected experts in ascending expert index, y = y + g_e * o_e from zero.  Each expert
    runs on its own rows only."""
    x = np.ascontiguousarray(x, f32)
    rows = x.shape[0]
    y = np.zeros((rows, experts[0][2].shape[0]), f32)
    for e, (W1, b1, W2, b2) in enumerate(experts):
        hit = sel == e
        idx = np.nonzero(hit.any(1))[0]
        if idx.size == 0:
            continue
        o = orc.linear(orc.linear(x[idx], W1, b1, relu=True), W2, b2)
        ge = g[idx, hit[idx].argmax(1)]
        y[idx] = (y[idx] + (ge[:, None] * o).astype(f32)).astype(f32)
    return y


def moe(x, w_gate, experts, k, w_noise=None, noise=None):
    """-> (MoE(x) [rows, E], p, sel, g)"""
    p, sel, g = gate(x, w_gate, k, w_noise, noise)
    return combine(x, experts, sel, g), p, sel, g


def sublayer(h, w_gate, experts, k, w_noise=None, noise=None, bn=None):
    """[BN_eval](h + MoE(h)) on rows [rows, E]; bn = (gamma, beta, mean, var, eps).  -> (out, p, sel, g)"""
    y, p, sel, g = moe(h, w_gate, experts, k, w_noise, noise)
    out = (np.ascontiguousarray(h, f32) + y).astype(f32)
    if bn is not None:
        out = orc.batchnorm_eval(out, *bn[:4], eps=bn[4])
    return out, p, sel, g


def encode(sd, env_name, locs, demand=None, k=2, num_heads=8):
    """oracle.encode's layer loop with the MoE sublayer -> (init embeddings, embeddings, per layer (h, p, sel, g))."""
    init_h, _ = orc.encode({key: v for key, v in sd.items() if ".net.layers." not in key}, env_name, locs, demand, num_heads)
    h = init_h.copy()
    per_layer = []
    layer = 0
    while f"encoder.net.layers.{layer}.0.module.Wqkv.weight" in sd:
        q = f"encoder.net.layers.{layer}."
        qkv = orc.linear(h, sd[q + "0.module.Wqkv.weight"], sd[q + "0.module.Wqkv.bias"])
        att = orc.mha_encoder(qkv, num_heads)
        h = h + orc.linear(att, sd[q + "0.module.out_proj.weight"], sd[q + "0.module.out_proj.bias"])
        h = orc._norm(sd, q + "1.normalizer.", h)
        B, M, E = h.shape
        y, p, sel, g = moe(h.reshape(B * M, E), sd[q + "2.module.w_gate"], experts_of(sd, q + "2.module."), k)
        h = (h + y.reshape(B, M, E)).astype(f32)
        h = orc._norm(sd, q + "3.normalizer.", h)
        per_layer.append((h.copy(), p, sel, g))
        layer += 1
    return init_h, h, per_layer


def policy_rollout(sd, env_name, locs, demand=None, decode_type="greedy", num_starts=0, noise=None, given=None,
                   use_graph_context=True, k=2, num_heads=8):
    """oracle.policy_rollout around `encode` -> dict(actions, logp_steps, log_likelihood, reward, embeddings, layers)."""
    _, emb, per_layer = encode(sd, env_name, locs, demand, k, num_heads)
    cache = orc.precompute(sd, env_name, emb, use_graph_context)
    multistart = "multistart" in decode_type and num_starts > 1
    st = orc.State(env_name, locs, demand, num_starts=num_starts if multistart else 0)
    mode = "evaluate" if given is not None else ("greedy" if "greedy" in decode_type else "sampling")
    pre_a, pre_lp = [], []
    if multistart:
        nloc = st.M if env_name == "tsp" else st.M - 1
        start = (np.repeat(np.arange(num_starts), st.Binst) % nloc + (0 if env_name == "tsp" else 1)).astype(np.int64)
        if given is not None:
            start, given = np.ascontiguousarray(given[:, 0]), np.ascontiguousarray(given[:, 1:])
        st.step(start)
        pre_a, pre_lp = [start[:, None]], [np.zeros((st.R, 1), f32)]
    acts, lps = orc.rollout(st, cache, mode, noise=noise, given=given, num_heads=num_heads)
    actions = np.ascontiguousarray(np.concatenate(pre_a + [acts], 1))
    logp = np.ascontiguousarray(np.concatenate(pre_lp + [lps], 1))
    return {"actions": actions, "logp_steps": logp, "log_likelihood": orc.sum_logp(logp),
            "reward": orc.tour_length_reward(locs, actions, with_depot=(env_name != "tsp")), "embeddings": emb,
            "layers": per_layer}


def run_fixture(fx):
    decode_type = str(fx["decode_type"])
    return policy_rollout(weights(cfg_for(fx), fx), str(fx["env_name"]), fx["locs"], fx.get("demand"), decode_type=decode_type,
                          num_starts=int(fx["num_starts"]), noise=fx.get("noise"),
                          given=fx["actions"] if decode_type == "evaluate" else None,
                          use_graph_context=bool(fx.get("policy_kw_use_graph_context", True)), k=int(fx["k"]))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(fixture, moe_ref's result on it), computed once per session; treat both as read-only."""
    fx = golden(name)
    return fx, run_fixture(fx)
