"""A plain restatement of the EAS-Lay layer (struct eamrl_eas_layer, include/eamrl.h) and of the decode step around it, in torch
on the CPU, built on tests/reeval_ref.py.

Written from the header's contract and the reference lines it names (zoo/eas/nn.py:5-30, zoo/eas/decoder.py:12-32), not from the
kernels.  Per (row r, step t), row r belonging to instance b = r % B, with h the glimpse output (concatenated heads):

    pre = h W1[b] + b1[b];   a = relu(pre);   y = h + a W2[b] + b2[b]
    u[n] = y . Lp[b][n] / sqrt(128);   z = clip tanh(u) (u when clip = 0), infeasible n -> -inf, / temp;   logp = z[a] - logsumexp(z)

Steps t < tstart give log-prob 0 and no gradient.  Gradients are torch autograd's of sum(glogp * logp) with respect to the four
layer parameters.  The functions compute in the dtype they are handed: float64 is the reference, the float32 run gives the scale
of float32 rounding (tests/eas_layer_cases.py)."""
import math

import torch

import reeval_ref as rr

E = rr.E
PARAMS = ("W1", "b1", "W2", "b2")
GRADS = ("dW1", "db1", "dW2", "db2")


def layer(h, lay, inst):
    """h [R, T, E]; lay: W1, W2 [N, E, E], b1, b2 [N, E]; inst [R] -> (y, pre)."""
    pre = torch.einsum("rte,ren->rtn", h, lay["W1"][inst]) + lay["b1"][inst][:, None, :]
    a = torch.relu(pre)
    return h + torch.einsum("rte,ren->rtn", a, lay["W2"][inst]) + lay["b2"][inst][:, None, :], pre


def pointer_logits(heads, lay, Wout, logit_key):
    """The reference's pointer with the layer and the UNFOLDED logit key (zoo/eas/decoder.py:12-32): heads [N, Q, E] of N
    instances, Wout = project_out.weight, logit_key [N, M, E] -> raw logits [N, Q, M]."""
    y, _ = layer(heads, lay, torch.arange(heads.shape[0]))
    glimpse = y @ Wout.t()
    return torch.einsum("nqe,nme->nqm", glimpse, logit_key) / math.sqrt(E)


def forward(op, lay, heads):
    """op: Lp [B, M, E], mask [R, T, M] bool, actions [R, T], S, tstart, clip, temp (tests/reeval_cases.py); heads [R, T, E]
    -> dict of logp, lse [R, T] (0 at steps t < tstart), pre, y [R, T, E], u [R, T, M], active [R, T]."""
    Lp, mask, actions = op["Lp"], op["mask"], op["actions"]
    B = Lp.shape[0]
    R, T = actions.shape
    inst = torch.arange(R) % B
    active = (torch.arange(T) >= op["tstart"])[None, :].expand(R, T)
    mask = mask | ~active[:, :, None]
    y, pre = layer(heads, lay, inst)
    u = torch.einsum("rte,rne->rtn", y, Lp[inst]) / math.sqrt(E)
    z = op["clip"] * torch.tanh(u) if op["clip"] > 0 else u
    zt = (z / op["temp"]).masked_fill(~mask, -math.inf)
    lse = torch.logsumexp(zt, dim=-1)
    logp = zt.gather(-1, actions[..., None]).squeeze(-1) - lse
    zero = torch.zeros_like(lse)
    return dict(logp=torch.where(active, logp, zero), lse=torch.where(active, lse, zero), pre=pre, y=y, u=u, active=active)


def cast(lay, dtype):
    return {k: v.to(dtype) for k, v in lay.items()}


def with_grads(op, lay, heads, glogp, dtype=torch.float64):
    """Values and autograd gradients of sum(glogp * logp) with every floating operand in `dtype` -> forward's dict + dW1 db1 dW2 db2."""
    lay = {k: v.to(dtype).detach().clone().requires_grad_() for k, v in lay.items()}
    out = forward(rr.cast(op, dtype), lay, heads.to(dtype))
    (glogp.to(dtype) * out["logp"]).sum().backward()
    res = {k: v.detach() for k, v in out.items()}
    for k in PARAMS:
        res["d" + k] = lay[k].grad if lay[k].grad is not None else torch.zeros_like(lay[k])
    return res
