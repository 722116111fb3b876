"""The yardstick of the PolyNet tests: one decode step of the PolyNet decoder restated in numpy / float64.

    heads  = inner masked MHA(query, K, V)                      (AttentionModelDecoder.forward, zoo/am/decoder.py:161-198)
    g      = heads Wout^T                                       (PolyNetAttention.forward, nn/attention.py:519-556)
    h      = relu(W1 [g ; z_j] + b1)
    y      = g + (W2 h + b2)
    logits = y . L[n] / sqrt(E) -> tanh clip -> mask -> / temperature -> log-softmax

Row r = s * B + b of a rollout with S rows per instance belongs to instance b and uses strategy j = s % k.  The env side (masks, first / current
node, used capacity) is replayed from the actions with tests/step_ref.py.  Operands are the float32 tensors handed in (weights, node
embeddings and, where given, the cache's own K / V / L / graph context); every operation on them is float64.

tests/test_host_polynet.py pins this module to the per-step log-probs recorded from the reference; tests/test_gpu_polynet.py holds
the rollout kernel to it.
"""
from __future__ import annotations

import functools
import itertools
import json
import math
import os

import numpy as np

import goldweights
import step_ref
from _util import GOLDEN, golden

E, H, P = 128, 8, 256

ROLLOUT_FIXTURES = ["polynet_tsp20_k5_s7_greedy", "polynet_tsp20_k2_s17_greedy", "polynet_tsp20_k1_s3_greedy",
                    "polynet_tsp20_k5_s7_samples_greedy",
                    "polynet_cvrp20_k8_s8_sampling", "polynet_cvrp20_k8_s8_evaluate", "polynet_tsp100_k128_s128_greedy",
                    "polynet_tsp101_k16_s16_greedy", "polynet_tsp112_k16_s16_greedy"]

with open(os.path.join(GOLDEN, "state_dict_contract_polynet.json")) as _f:
    CONTRACT = json.load(_f)


def binary_vectors(k):
    """The first k of itertools.product([0, 1], repeat=ceil(log2 k)) as [k, dz] float32."""
    dz = math.ceil(math.log2(k))
    return np.array(list(itertools.product([0, 1], repeat=dz))[:k], np.float32).reshape(k, dz)


def weights(env_name, k):
    """{key: float32 ndarray}: the closed-form weights of the contract's entries, the strategy table left as the model defines it."""
    sd = {}
    dz = math.ceil(math.log2(k))
    # (a k the contract file does not list: its entries are those of any other k but for the width of the strategy vector)
    for key, shape, dt in CONTRACT.get(f"polynet_{env_name}_k{k}", CONTRACT[f"polynet_{env_name}_k2"]):
        if dt != "float32":
            continue
        if key.endswith("binary_vectors"):
            sd[key] = binary_vectors(k)
            continue
        if key.endswith("poly_layer_1.weight"):
            shape = [shape[0], E + dz]
        v = goldweights.tensor_for(key, shape)
        if v is not None:
            sd[key] = v
    return sd


def batch_of(fx):
    """step_ref's batch dict of a fixture (CVRP: locs carry the depot first; capacity is 1 after the generator's normalisation)."""
    env_name = str(fx["env_name"])
    if env_name == "tsp":
        return {"env": "tsp", "locs": fx["locs"]}
    return {"env": "cvrp", "locs": fx["locs"][:, 1:], "depot": fx["locs"][:, 0], "demand": fx["demand"]}


def cache_of(sd, emb):
    """K, V, L and the graph context from the node embeddings (AttentionModelDecoder._precompute_cache, decoder.py:206-235)."""
    emb = np.asarray(emb, np.float64)
    kvl = emb @ sd["decoder.project_node_embeddings.weight"].astype(np.float64).T
    return {"emb": emb, "K": kvl[..., :E], "V": kvl[..., E:2 * E], "L": kvl[..., 2 * E:],
            "gctx": emb.mean(1) @ sd["decoder.project_fixed_context.weight"].astype(np.float64).T}


def step_logprobs(sd, cache, env_name, states, k, s_first=0, clip=10.0, temp=1.0):
    """Log-probs [R, M] (float64, -inf where masked) of one decode step for the R = S * B rows whose step_ref states are
    `states` ((s b) order); rows that are done get a row of zeros."""
    f8 = lambda x: np.asarray(x, np.float64)
    emb, K, V, L, gctx = (f8(cache[n]) for n in ("emb", "K", "V", "L", "gctx"))
    B, M, _ = emb.shape
    R = len(states)
    b = np.arange(R) % B
    cur = np.array([s["cur"] for s in states])
    mask = np.stack([s["mask"] for s in states])
    done = np.array([bool(s["done"]) for s in states])
    Wctx = f8(sd["decoder.context_embedding.project_context.weight"])
    if env_name == "tsp":
        first = np.array([s["first"] for s in states])
        ctx = np.concatenate([emb[b, first], emb[b, cur]], -1)
        fresh = np.array([s["istep"] == 0 for s in states])
        ctx[fresh] = f8(sd["decoder.context_embedding.W_placeholder"])
    else:
        free = np.array([np.float64(s["vcap"]) - np.float64(s["used"]) for s in states])
        ctx = np.concatenate([emb[b, cur], free[:, None]], -1)
    q = ctx @ Wctx.T + gctx[b]
    D = E // H
    qh = q.reshape(R, H, D)
    kh = K[b].reshape(R, M, H, D)
    vh = V[b].reshape(R, M, H, D)
    sc = np.einsum("rhd,rmhd->rhm", qh, kh) / math.sqrt(D)
    sc = np.where(mask[:, None, :], sc, -np.inf)
    sc = sc - sc.max(-1, keepdims=True)
    w = np.exp(sc)
    w = w / w.sum(-1, keepdims=True)
    heads = np.einsum("rhm,rmhd->rhd", w, vh).reshape(R, E)
    g = heads @ f8(sd["decoder.pointer.project_out.weight"]).T
    Z = f8(sd["decoder.pointer.binary_vectors"])
    z = Z[(s_first + np.arange(R) // B) % k]
    hid = np.maximum(np.concatenate([g, z], -1) @ f8(sd["decoder.pointer.poly_layer_1.weight"]).T
                     + f8(sd["decoder.pointer.poly_layer_1.bias"]), 0.0)
    y = g + (hid @ f8(sd["decoder.pointer.poly_layer_2.weight"]).T + f8(sd["decoder.pointer.poly_layer_2.bias"]))
    logits = np.einsum("re,rme->rm", y, L[b]) / math.sqrt(E)
    if clip > 0:
        logits = np.tanh(logits) * clip
    logits = np.where(mask, logits, -np.inf) / temp
    mx = logits.max(-1, keepdims=True)
    lp = logits - (mx + np.log(np.exp(logits - mx).sum(-1, keepdims=True)))
    lp[done] = 0.0
    return lp


def rollout_logp(sd, cache, batch, actions, k, s_first=0, clip=10.0, temp=1.0, forced_start=False):
    """Selected log-probs [R, T] (float64) of the action rows [R, T] ((s b) order).  forced_start: column 0 is the start node of a
    multistart rollout -- no decision, log-prob 0 (utils/decoding.py:306-324); otherwise every column is a decision."""
    actions = np.asarray(actions)
    R, T = actions.shape
    B = step_ref.num_instances(batch)
    env_name = str(batch["env"])
    states = step_ref.reset_rows(batch, R // B)
    out = np.zeros((R, T), np.float64)
    for t in range(T):
        if not (forced_start and t == 0):
            lp = step_logprobs(sd, cache, env_name, states, k, s_first, clip, temp)
            live = np.array([not s["done"] for s in states])
            out[live, t] = lp[np.arange(R), actions[:, t]][live]
        states = [step_ref.step(s, a) if not s["done"] else s for s, a in zip(states, actions[:, t])]
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(fixture, weights, float64 selected log-probs [R, T] of the fixture's own actions from its recorded embeddings): computed
    once per fixture and shared by the tests; read-only."""
    fx = golden(name)
    k, env_name = int(fx["k"]), str(fx["env_name"])
    sd = weights(env_name, k)
    lp = rollout_logp(sd, cache_of(sd, fx["embeddings"]), batch_of(fx), fx["actions"], k, forced_start=bool(fx["forced_start"]))
    lp.setflags(write=False)
    return fx, sd, lp
