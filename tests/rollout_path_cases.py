"""The cases of tests/test_gpu_rollout_paths.py and tests/golden/make_golden_rollout_paths.py: one tiny rollout per branch of
the whole-rollout call path (ops.rollout -> eamrl_am_rollout*), on synthetic decoder caches drawn from a CPU generator.

B = 3 instances, embed_dim 128, 8 heads; TSP with 9 nodes, CVRP with 9 customers (10 nodes).  Every tensor a case reads comes from
`torch.Generator().manual_seed(...)` on the CPU and pure indexing, so the inputs are the same bits on every machine; the outputs
are compared bit for bit with what the recorded build returned (tests/golden/rollout_paths.npz).

`run(name)` -> {key: numpy array}: actions, logps (int32 bit patterns), info, the final mask and cur, and for the EAS-Lay cases the
captured pre-layer heads (bit patterns).  It asserts that the case lands on the kernel it is meant to cover.
"""
import ctypes as C
import functools

import numpy as np
import torch

DEV = "cuda"
B, E, H, K_POLY, P_POLY = 3, 128, 8, 4, 256
ENVS = ("tsp", "cvrp")
NODES = {"tsp": 9, "cvrp": 10}
SEED = 20250917

# name -> (kind, rows per instance, kernel ops.rollout_kernel must name for the call's shape and filter)
KINDS = {
    "greedy_resident": (1, "resident"),         # greedy single rows
    "greedy_stream": (1, "stream"),             # the same with debug key 1
    "seeded_ms": (4, "ms_mfma"),                # multistart, sampling with a seed: in-place noise
    "seeded_single": (1, "resident"),           # the same seed on single rows: scratch-noise fallback
    "seeded_topk3": (4, "resident"),            # seed + top_k = 3: noise materialised in Python, filtering variant
    "evaluate_given": (1, "resident"),          # evaluate the greedy tours
    "polynet_noise": (4, "ms_mfma"),            # PolyNet, k = 4, noise tensor
    "polynet_seeded": (4, "ms_mfma"),           # PolyNet, k = 4, seed
    "eas_layer_seeded": (4, "ms_mfma"),         # EAS-Lay: seed, forced last row, captured heads
}
NAMES = [f"{env}_{kind}" for env in ENVS for kind in KINDS]


@functools.lru_cache(maxsize=None)
def operands(env):
    """CPU tensors of one env's cases, drawn once in a fixed order."""
    M = NODES[env]
    g = torch.Generator().manual_seed(SEED + (env == "cvrp"))
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    slots = 6 if env == "tsp" else 5
    o = {"buf": rn(B, M, slots * E, scale=0.5), "cvec": rn(E, scale=0.5), "gctx": rn(B, E, scale=0.5)}
    if env == "cvrp":
        o["demand"] = (torch.randint(1, 10, (B, M - 1), generator=g).float() / 30.0).contiguous()
    o["noise"] = -torch.log(torch.rand(4 * B, 2 * M + 1, M, generator=g).clamp_min(1e-30))        # Exp(1), [R, T, M]
    o["poly"] = {"Wout": rn(E, E, scale=E ** -0.5), "W1": rn(P_POLY, E, scale=E ** -0.5), "ctab": rn(K_POLY, P_POLY, scale=0.3),
                 "W2": rn(E, P_POLY, scale=P_POLY ** -0.5), "b2": rn(E, scale=0.1)}
    o["layer"] = {"W1": rn(B, E, E, scale=0.1), "b1": rn(B, E, scale=0.3), "W2": rn(B, E, E, scale=0.05), "b2": rn(B, E, scale=0.1)}
    return o


def cache_of(env):
    from eam_rl4co_amd import ops

    o = operands(env)
    d = lambda x: x.to(DEV).contiguous()
    return ops.DecodeCache(env, d(o["buf"]), d(o["cvec"]), d(o["gctx"]), None, H, embed_dim=E)


def state_of(env, S):
    """The reset state of R = S * B rows; with S > 1 after the multistart step (row s * B + b starts at node s, CVRP: customer s + 1)."""
    from eam_rl4co_amd import ops
    from eam_rl4co_amd.policy import _env_step_

    o = operands(env)
    st = ops.RolloutState(env, S * B, NODES[env], DEV, demand=o["demand"].to(DEV) if env == "cvrp" else None)
    if S > 1:
        start = (torch.arange(S, device=DEV) + (env == "cvrp")).repeat_interleave(B).contiguous()
        _env_step_(st, start)
    return st


def _out(st, actions, logps, info):
    return {"actions": actions.cpu().numpy(), "logps": logps.cpu().numpy().view(np.int32), "info": info.cpu().numpy(),
            "mask": st.mask.cpu().numpy().astype(np.uint8), "cur": st.cur.cpu().numpy()}


def run(name):
    from eam_rl4co_amd import _lib, env_spec, ops

    env, kind = name.split("_", 1)
    S, kernel = KINDS[kind]
    o, M = operands(env), NODES[env]
    cache, st = cache_of(env), state_of(env, S)
    t_max = env_spec.max_steps(env, M, 1 if S > 1 else 0)
    kw = dict(clip=10.0, temp=1.0, t_max=t_max)
    top_k = 3 if kind == "seeded_topk3" else 0
    lib = _lib.load()
    forced = kind == "greedy_stream"
    try:
        if forced:
            assert lib.eamrl_debug_set(1, 1) == 0
        assert ops.rollout_kernel(st, cache, st.R, t_max, top_k=top_k) == kernel, name
        if kind in ("greedy_resident", "greedy_stream"):
            res = ops.rollout(st, cache, "greedy", **kw)
        elif kind in ("seeded_ms", "seeded_single", "seeded_topk3"):
            cs = cache.struct()
            assert bool(lib.eamrl_rollout_rng_native(ops.ENVS[env], C.byref(cs), st.R)) == (kind != "seeded_single")
            res = ops.rollout(st, cache, "sampling", seed=977, top_k=top_k, **kw)
        elif kind == "evaluate_given":
            acts, _, info = ops.rollout(state_of(env, S), cache, "greedy", **kw)
            given = acts[:, :int(info[0])].contiguous()
            res = ops.rollout(st, cache, "evaluate", given=given, **kw)
        elif kind in ("polynet_noise", "polynet_seeded"):
            poly = {n: (ops.pack_mfma_a(v) if v.dim() == 2 and n != "ctab" else v.clone()).to(DEV).contiguous() for n, v in o["poly"].items()}
            poly.update(k=K_POLY, P=P_POLY)
            how = dict(seed=977) if kind == "polynet_seeded" else dict(noise=o["noise"][:, :t_max].to(DEV).contiguous())
            res = ops.rollout(st, cache, "sampling", poly=poly, **how, **kw)
        else:
            # the forced tour of every instance's last row: what the plain seeded rollout took on that row (same start node)
            acts, _, info = ops.rollout(state_of(env, S), cache, "sampling", seed=977, **kw)
            tour = acts[(S - 1) * B:, :int(info[0])].contiguous()
            layer = ops.eas_layer_operands(*(o["layer"][n].to(DEV) for n in ("W1", "b1", "W2", "b2")), forced=tour)
            res = ops.rollout(st, cache, "sampling", seed=31, want_heads=True, eas_layer=layer, **kw)
    finally:
        if forced:
            lib.eamrl_debug_set(1, 0)
    out = _out(st, *res)
    if kind == "eas_layer_seeded":
        assert st.heads is not None
        out["heads"] = st.heads.cpu().numpy().view(np.int32)
    return out
