"""A plain restatement of the teacher-forced re-evaluation operator (struct eamrl_reeval, include/eamrl.h), in torch on the CPU.

Written from the header's contract and the reference lines it names -- `policy(td, env, actions=...)` with decode type
"evaluate" (models/common/constructive/base.py:203-229, utils/decoding.py:452-465), the decoder's pointer attention
(models/zoo/am/decoder.py:133-198, models/nn/attention.py:282-328), the logit processing (utils/decoding.py:140-190), the
entropy (utils/ops.py calculate_entropy) and SDVRP's dynamic embedding (models/nn/env_embeddings/dynamic.py:59-78) -- not
from the kernels.  Per (row r, step t), row r belonging to instance r % B:

    q      = Pa[idxA] + Pb[idxB] + gctx + sum_k sc_k Cvec_k            (an index of -1 contributes nothing)
    heads  = eight heads of 16: softmax(q_h . K_h[n] / 4 over the feasible n) V_h
    u[n]   = heads . Lp[n] / sqrt(128)
    z[n]   = clip tanh(u[n]) (u[n] when clip = 0), infeasible n -> -inf, then / temp
    lse    = logsumexp(z);  logp = z[a] - lse;  entropy = -sum_n p[n] log p[n] over the feasible n, p = exp(z - lse)

Steps t < tstart give log-prob 0, entropy 0 and no gradient.  SDVRP (dyn = wk | wv | lw, rem [R, T, M]) adds
rem[n] * (wk | wv | lw) to row n of K / V / Lp at that step.  Gradients are torch autograd's of sum(glogp * logp).  The functions
compute in the dtype of K: float64 is the reference, the float32 run gives the scale of float32 rounding (tests/reeval_cases.py).

`mutant` selects a deliberately wrong one-line variant (tests/test_host_reeval_ref.py shows that the case list sees each).
"""
import math

import numpy as np
import torch

E, H, D = 128, 8, 16
KEY_CHUNK = 112
MUTANTS = ("instance_r_div_S", "tstart_ignored", "idxB_ignored", "temp_dropped_in_grad", "tanh_derivative_dropped",
           "glimpse_unmasked", "entropy_from_unclipped", "rem_of_previous_step")
GRADS = ("dK", "dV", "dLp", "dPa", "dPb", "dgctx", "dCvec", "ddyn")


def glimpse_logits(q, K, V, Lp, mask, glimpse_mask=True):
    """q [R, T, E]; K / V / Lp [R, M, E] or (per step) [R, T, M, E]; mask [R, T, M] bool -> heads [R, T, E], u [R, T, M],
    attention weights [R, T, H, M]."""
    R, T, _ = q.shape
    per_step = K.dim() == 4
    kv = "rtnhd" if per_step else "rnhd"
    split = (lambda x: x.reshape(*x.shape[:-1], H, D))
    s = torch.einsum(f"rthd,{kv}->rthn", split(q), split(K)) / 4.0            # 1 / sqrt(16)
    if glimpse_mask:
        s = s.masked_fill(~mask[:, :, None, :], -math.inf)
    a = torch.softmax(s, dim=-1)
    heads = torch.einsum(f"rthn,{kv}->rthd", a, split(V)).reshape(R, T, E)
    u = torch.einsum("rte,rtne->rtn" if per_step else "rte,rne->rtn", heads, Lp) / math.sqrt(E)
    return heads, u, a


def reeval(op, mutant=None):
    """op: dict of K, V, Lp, Pa [B, M, E]; Pb or None; gctx [B, E] or None; Cvec [NC, E] or None; sc [NC, R, T]; idxA, idxB
    [R, T] (idxB with Pb only); mask [R, T, M] bool; actions [R, T]; S, tstart, clip, temp; rem [R, T, M], dyn [3, E] or None;
    heads [R, T, E] or None (given glimpse outputs, used instead of the recomputed ones).
    -> dict of logp, lse, entropy [R, T] (0 at steps t < tstart), heads [R, T, E], u [R, T, M], attn [R, T, H, M]."""
    assert mutant is None or mutant in MUTANTS
    K, V, Lp, Pa = op["K"], op["V"], op["Lp"], op["Pa"]
    B, M, _ = K.shape
    actions, mask = op["actions"], op["mask"]
    R, T = actions.shape
    S, clip, temp = op["S"], op["clip"], op["temp"]
    tstart = 0 if mutant == "tstart_ignored" else op["tstart"]
    assert R == S * B
    rows = torch.arange(R)
    inst = rows // S if mutant == "instance_r_div_S" else rows % B
    active = (torch.arange(T) >= tstart)[None, :].expand(R, T)
    mask = mask | ~active[:, :, None]              # (inactive steps: any mask will do, their results are discarded)

    def rows_of(P, idx):
        return P[inst[:, None], idx.clamp(min=0).long()] * (idx >= 0)[:, :, None].to(P.dtype)

    q = rows_of(Pa, op["idxA"])
    if op.get("Pb") is not None and mutant != "idxB_ignored":
        q = q + rows_of(op["Pb"], op["idxB"])
    if op.get("gctx") is not None:
        q = q + op["gctx"][inst][:, None, :]
    if op.get("Cvec") is not None:
        q = q + torch.einsum("krt,ke->rte", op["sc"], op["Cvec"])

    Kr, Vr, Lr = K[inst], V[inst], Lp[inst]
    if op.get("dyn") is not None:
        rem = op["rem"]
        if mutant == "rem_of_previous_step":
            rem = torch.cat([rem[:, :1], rem[:, :-1]], dim=1)
        wk, wv, lw = op["dyn"]
        Kr, Vr, Lr = (X[:, None] + rem[..., None] * w for X, w in ((Kr, wk), (Vr, wv), (Lr, lw)))
    heads, u, attn = glimpse_logits(q, Kr, Vr, Lr, mask, glimpse_mask=mutant != "glimpse_unmasked")
    if op.get("heads") is not None:
        heads = heads + (op["heads"] - heads).detach()      # the given values; the gradient is that of the glimpse they came from
        u = torch.einsum("rte,rtne->rtn" if Lr.dim() == 4 else "rte,rne->rtn", heads, Lr) / math.sqrt(E)

    if clip > 0:
        z = clip * torch.tanh(u)
        if mutant == "tanh_derivative_dropped":
            z = z.detach() + clip * (u - u.detach())
    else:
        z = u
    zt = z / temp
    if mutant == "temp_dropped_in_grad":
        zt = zt.detach() + (z - z.detach())
    zt = zt.masked_fill(~mask, -math.inf)
    lse = torch.logsumexp(zt, dim=-1)
    logp = zt.gather(-1, actions[..., None]).squeeze(-1) - lse
    logpn = zt - lse[..., None]
    entropy = -torch.where(mask, logpn.exp() * logpn, torch.zeros_like(logpn)).sum(-1)
    if mutant == "entropy_from_unclipped":
        entropy = lse - torch.where(mask, logpn.exp() * u / temp, torch.zeros_like(u)).sum(-1)
    zero = torch.zeros_like(lse)
    return dict(logp=torch.where(active, logp, zero), lse=torch.where(active, lse, zero),
                entropy=torch.where(active, entropy, zero).detach(), heads=heads, u=u, attn=attn, active=active)


DIFF = (("dK", "K"), ("dV", "V"), ("dLp", "Lp"), ("dPa", "Pa"), ("dPb", "Pb"), ("dgctx", "gctx"), ("dCvec", "Cvec"), ("ddyn", "dyn"))


def cast(op, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in op.items()}


def reeval_with_grads(op, glogp, dtype=torch.float64, mutant=None):
    """Values and autograd gradients of sum(glogp * logp) with every operand in `dtype`.
    -> dict of logp, lse, entropy, heads, u, attn and dK, dV, dLp, dPa, dPb, dgctx, dCvec, ddyn (absent operands are left out)."""
    op = cast(op, dtype)
    leaves = {}
    for g, name in DIFF:
        if op.get(name) is not None:
            op[name] = op[name].detach().clone().requires_grad_()
            leaves[g] = op[name]
    out = reeval(op, mutant)
    (glogp.to(dtype) * out["logp"]).sum().backward()
    res = {k: v.detach() for k, v in out.items()}
    for g, leaf in leaves.items():
        res[g] = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
    return res


# ---- the kernel's operand layouts --------------------------------------------------------------------------------------------
def pack_mask_bits(mask):
    """bool [R, T, M], M <= 128 -> int32 [R, T, 4]: bit n of the 128-bit word = node n feasible."""
    m = np.asarray(mask, dtype=bool)
    R, T, M = m.shape
    assert M <= 128
    pad = np.zeros((R, T, 128), dtype=np.uint32)
    pad[..., :M] = m
    words = (pad.reshape(R, T, 4, 32) << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint32)
    return torch.from_numpy(words.view(np.int32).copy())


def pack_mask_bits_chunked(mask):
    """bool [R, T, M] -> int32 [R, T, nkc, 4], nkc = ceil(M / 112): bit i of chunk c = node 112 c + i."""
    m = np.asarray(mask, dtype=bool)
    R, T, M = m.shape
    nkc = -(-M // KEY_CHUNK)
    pad = np.zeros((R, T, nkc * KEY_CHUNK), dtype=bool)
    pad[..., :M] = m
    return pack_mask_bits(pad.reshape(R, T * nkc, KEY_CHUNK)).reshape(R, T, nkc, 4)


def rem_rows(rem):
    """[R, T, M] -> [R, T, 128] (M <= 112) or [R, T, nkc, 128] (entry i of chunk c = node 112 c + i), zero padded, float32."""
    R, T, M = rem.shape
    nkc = -(-M // KEY_CHUNK)
    out = torch.zeros(R, T, nkc, 128, dtype=torch.float32)
    pad = torch.zeros(R, T, nkc * KEY_CHUNK, dtype=torch.float32)
    pad[..., :M] = rem.float()
    out[..., :KEY_CHUNK] = pad.reshape(R, T, nkc, KEY_CHUNK)
    return out[:, :, 0].contiguous() if nkc == 1 else out
