"""The yardstick of the pickup-and-delivery (PDP) tests, built from the CPU oracle as it stands.

Integer side -- reset, step, mask, done, start nodes, validity verdicts -- is plain numpy, restated from
rl4co/envs/routing/pdp/env.py:66-240.  Floating-point side is composed from `oracle.oracle` primitives:

  init embedding  three `linear` calls on the depot, pickup (x_p, y_p, x_d, y_d) and delivery features
  encoder         the layer loop of `oracle.encode`, restated with `linear`, `mha_encoder` and `_norm`
  cache           `oracle.precompute` in its depot-env form on a project_context widened by a zero state column, i.e. cvec = 0
  decode step     `oracle.decode_step` in its CVRP form on a duck-typed state whose mask the numpy state machine supplies, with
                  used = vcap = 0: the state term of the query is fma(0, 0 - 0, Pa[cur]), so the step is bit-defined
  reward          `oracle.tour_length_reward(with_depot=True)`

tests/test_host_pdp.py pins this module to the reference's recorded results; tests/test_gpu_pdp.py holds the HIP kernels to it
bit for bit.  Results per fixture are computed once (`reference`) and shared.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import goldweights
from _util import GOLDEN, golden
from oracle import oracle as orc

VALID, NOT_ALL_NODES, DELIVERY_FIRST = 0, 1, 2

ROLLOUT_FIXTURES = ["pdp4_greedy", "pdp20_greedy", "pdp20_sampling", "pdp20_evaluate", "pdp20_sampling_topk5",
                    "pdp20_sampling_topp09", "pomo_pdp20_multistart_greedy", "pdp110_greedy", "pdp126_greedy", "pdp128_greedy",
                    "pdp20_greedy_depot_start"]

with open(os.path.join(GOLDEN, "state_dict_contract_pdp.json")) as _f:
    CONTRACT = json.load(_f)


def weights(cfg):
    """{key: float32 ndarray} of the closed-form weights for "am_pdp" / "pomo_pdp"."""
    sd = {}
    for k, shape, dt in CONTRACT[cfg]:
        if dt == "float32":
            v = goldweights.tensor_for(k, shape)
            if v is not None:
                sd[k] = v
    return sd


def cfg_for(fx):
    return ("pomo_" if "policy_kw_num_encoder_layers" in fx else "am_") + "pdp"


# ---------------------------------------------------------------------------------------------------------------------
# integer side
# ---------------------------------------------------------------------------------------------------------------------
class Env:
    """PDPEnv's state for R rows: available, to_deliver, action_mask [R, M] bool, current_node [R], done [R]."""

    def __init__(self, R, num_loc, force_start_at_depot=False):
        assert num_loc % 2 == 0
        self.N, self.M, self.R = num_loc, num_loc + 1, R
        self.to_deliver = np.zeros((R, self.M), bool)
        self.to_deliver[:, :num_loc // 2 + 1] = True
        self.available = np.ones((R, self.M), bool)
        if force_start_at_depot:
            self.action_mask = np.zeros((R, self.M), bool)
            self.action_mask[:, 0] = True
        else:
            self.available[:, 0] = False
            self.action_mask = self.available & self.to_deliver
        self.current_node = np.zeros(R, np.int64)
        self.done = np.zeros(R, bool)

    def step(self, action):
        a = np.asarray(action, np.int64)
        r = np.arange(self.R)
        self.available[r, a] = False
        self.to_deliver[r, (a + self.N // 2) % (self.N + 1)] = True        # the reference's modulo, as it is
        self.action_mask = self.available & self.to_deliver
        self.done = np.count_nonzero(self.available, axis=-1) == 0
        self.current_node = a.copy()


def select_start_nodes(B, num_loc, num_starts):
    return (np.repeat(np.arange(num_starts), B) % (num_loc // 2) + 1).astype(np.int64)


def check_solution(actions, num_loc, force_start_at_depot=False):
    """Verdict per row: the first assertion of PDPEnv.check_solution_validity that the row fails."""
    actions = np.asarray(actions, np.int64)
    out = np.empty(actions.shape[0], np.int64)
    for i, row in enumerate(actions):
        a = row if force_start_at_depot else np.concatenate([[0], row])
        T = a.shape[0]
        if not np.array_equal(np.sort(a), np.arange(T)) or (a[1:-1] == 0).any():
            out[i] = NOT_ALL_NODES
            continue
        when = np.argsort(a, kind="stable")
        out[i] = VALID if (when[1:T // 2 + 1] < when[T // 2 + 1:]).all() else DELIVERY_FIRST
    return out


# ---------------------------------------------------------------------------------------------------------------------
# floating-point side
# ---------------------------------------------------------------------------------------------------------------------
def init_embedding(sd, locs):
    locs = np.ascontiguousarray(locs, np.float32)
    half = (locs.shape[1] - 1) // 2
    pre = "encoder.init_embedding."
    depot = orc.linear(locs[:, :1], sd[pre + "init_embed_depot.weight"], sd[pre + "init_embed_depot.bias"])
    pick_feat = np.concatenate([locs[:, 1:half + 1], locs[:, half + 1:]], -1)
    pick = orc.linear(pick_feat, sd[pre + "init_embed_pick.weight"], sd[pre + "init_embed_pick.bias"])
    deliv = orc.linear(locs[:, half + 1:], sd[pre + "init_embed_delivery.weight"], sd[pre + "init_embed_delivery.bias"])
    return np.concatenate([depot, pick, deliv], 1)


def encode(sd, locs, num_heads=8):
    """-> (init embeddings, embeddings): the layer loop of oracle.encode."""
    h = init_embedding(sd, locs)
    init_h = h.copy()
    layer = 0
    while f"encoder.net.layers.{layer}.0.module.Wqkv.weight" in sd:
        p = f"encoder.net.layers.{layer}."
        qkv = orc.linear(h, sd[p + "0.module.Wqkv.weight"], sd[p + "0.module.Wqkv.bias"])
        att = orc.mha_encoder(qkv, num_heads)
        h = h + orc.linear(att, sd[p + "0.module.out_proj.weight"], sd[p + "0.module.out_proj.bias"])
        h = orc._norm(sd, p + "1.normalizer.", h)
        f = orc.linear(h, sd[p + "2.module.lins.0.weight"], sd[p + "2.module.lins.0.bias"], relu=True)
        h = h + orc.linear(f, sd[p + "2.module.lins.1.weight"], sd[p + "2.module.lins.1.bias"])
        h = orc._norm(sd, p + "3.normalizer.", h)
        layer += 1
    return init_h, h


def precompute(sd, emb, use_graph_context=True):
    key = "decoder.context_embedding.project_context.weight"
    W = np.asarray(sd[key], np.float32)
    wide = dict(sd)
    wide[key] = np.concatenate([W, np.zeros((W.shape[0], 1), np.float32)], 1)       # the state column a depot env has: zeros
    cache = orc.precompute(wide, "cvrp", emb, use_graph_context)
    assert not cache["cvec"].any()
    return cache


class DecodeState:
    """What oracle.decode_step reads, in its CVRP form: the mask comes from `Env`, used = vcap = 0."""

    def __init__(self, env: Env, binst):
        self.env_state = env
        self.env = orc.ENV_CVRP
        self.R, self.M, self.Binst = env.R, env.M, binst
        self.first = np.zeros(env.R, np.int64)
        self.istep = np.ones(env.R, np.int64)
        self.used = np.zeros(env.R, np.float32)
        self.vcap = np.zeros(env.R, np.float32)
        self.rem = self.time = None

    @property
    def cur(self):
        return np.ascontiguousarray(self.env_state.current_node, np.int64)

    @property
    def mask(self):
        return np.ascontiguousarray(self.env_state.action_mask, np.uint8)


def rollout(env: Env, binst, cache, mode="greedy", noise=None, given=None, clip=10.0, temp=1.0, num_heads=8, top_k=0,
            top_p=0.0, want_all=False):
    """Decode loop until every row is done -> (actions [R, T], logp [R, T][, logits, logprobs, masks per step])."""
    st = DecodeState(env, binst)
    acts, lps, extra = [], [], []
    t = 0
    while not env.done.all():
        assert t <= env.M, "rollout exceeded the number of nodes"
        mask = env.action_mask.copy()
        res = orc.decode_step(st, cache, mode, noise=None if noise is None else noise[:, t],
                              given=None if given is None else given[:, t], clip=clip, temp=temp, num_heads=num_heads,
                              want_all=want_all, top_k=top_k, top_p=top_p)
        if want_all:
            extra.append((res[2], res[3], mask))
        acts.append(res[0])
        lps.append(res[1])
        env.step(res[0])
        t += 1
    out = (np.stack(acts, 1), np.stack(lps, 1).astype(np.float32))
    return out + (extra,) if want_all else out


def policy_rollout(sd, locs, decode_type="greedy", num_starts=0, noise=None, given=None, use_graph_context=True, clip=10.0,
                   temp=1.0, num_heads=8, top_k=0, top_p=0.0, force_start_at_depot=False, want_all=False):
    """ConstructivePolicy.forward restated -> dict(actions, logp_steps, log_likelihood, reward, init_embeds, steps)."""
    locs = np.ascontiguousarray(locs, np.float32)
    B, M = locs.shape[:2]
    init_h, emb = encode(sd, locs, num_heads)
    cache = precompute(sd, emb, use_graph_context)
    multistart = "multistart" in decode_type and num_starts > 1
    S = num_starts if multistart else 1
    env = Env(B * S, M - 1, force_start_at_depot)
    mode = "evaluate" if given is not None else ("greedy" if "greedy" in decode_type else "sampling")
    pre_a, pre_lp = [], []
    if multistart:
        start = select_start_nodes(B, M - 1, S)
        if given is not None:
            start, given = np.ascontiguousarray(given[:, 0]), np.ascontiguousarray(given[:, 1:])
        env.step(start)
        pre_a, pre_lp = [start[:, None]], [np.zeros((env.R, 1), np.float32)]
    res = rollout(env, B, cache, mode, noise=noise, given=given, clip=clip, temp=temp, num_heads=num_heads, top_k=top_k,
                  top_p=top_p, want_all=want_all)
    actions = np.ascontiguousarray(np.concatenate(pre_a + [res[0]], 1))
    logp = np.ascontiguousarray(np.concatenate(pre_lp + [res[1]], 1))
    out = {"actions": actions, "logp_steps": logp, "log_likelihood": orc.sum_logp(logp),
           "reward": orc.tour_length_reward(locs, actions, with_depot=True), "init_embeds": init_h, "embeddings": emb,
           "final_available": env.available.copy(), "final_to_deliver": env.to_deliver.copy()}
    if want_all:
        out["steps"] = res[2]
    return out


def run_fixture(fx, want_all=False):
    decode_type = str(fx["decode_type"])
    ns = int(fx["num_starts"])
    return policy_rollout(
        weights(cfg_for(fx)), fx["locs"], decode_type=decode_type, num_starts=ns, noise=fx.get("noise"),
        given=fx["actions"] if decode_type == "evaluate" else None,
        use_graph_context=bool(fx.get("policy_kw_use_graph_context", True)),
        clip=float(fx.get("decode_kw_tanh_clipping", 10.0)), temp=float(fx.get("decode_kw_temperature", 1.0)),
        top_k=int(fx.get("decode_kw_top_k", 0)), top_p=float(fx.get("decode_kw_top_p", 0.0)),
        force_start_at_depot=bool(fx["force_start_at_depot"]), want_all=want_all)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(fixture, pdp_ref's result on it), computed once per session; treat both as read-only."""
    fx = golden(name)
    return fx, run_fixture(fx, want_all=True)
