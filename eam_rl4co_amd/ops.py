"""torch.Tensor front-end of the C ABI: checks device / dtype / contiguity / shapes on the host (a kernel
that faults can reset the GPU host) and enqueues on torch's current HIP stream.  Tensors are plumbing only:
every computation below happens in libeamrl_hip.so."""
from __future__ import annotations

import ctypes as C
import logging
import os

import torch

from . import _lib, env_spec
from ._lib import (ENV_CVRP, ENV_CVRPTW, ENV_OP, ENV_PCTSP, ENV_PDP, ENV_SDVRP, ENV_TSP, EVALUATE, GREEDY, NORM_BATCH_EVAL, NORM_INSTANCE, SAMPLE,  # noqa: F401
                   ST_INFEASIBLE, ST_NAN_LOGITS, ST_STEP_OVERRUN)

MODES = {"greedy": GREEDY, "sampling": SAMPLE, "evaluate": EVALUATE}
ENVS = {name: spec.abi_id for name, spec in env_spec.ENV_SPECS.items()}


def _need_gpu(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on {t.device}: the eam_rl4co_amd rollout path runs only on an MI355X (HIP) device; "
            "there is no CPU fallback. Move the TensorDict / policy to 'cuda'.")


def _chk(t, name, dtype, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    _need_gpu(t, name)
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _bytes(t):
    """bool tensors are passed as their uint8 storage; None stays None."""
    return t.view(torch.uint8) if t is not None and t.dtype == torch.bool else t


# ------------------------------------------------------------------------------------------------------
# encoder / cache
# ------------------------------------------------------------------------------------------------------
def _linear_views(x, W, residual, out, w_cols):
    """The 2-D operand views eamrl_linear is handed: (x2, Wv, res2, out, o2).  x is copied if its inner stride is not 1; W, the
    residual and `out` must have unit inner stride; `out` is allocated when None."""
    _need_gpu(x, "x")
    in_dim = x.shape[-1] if w_cols is None else w_cols[1] - w_cols[0]
    x2 = x.reshape(-1, x.shape[-1])
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    if W.dtype != torch.float32 or W.stride(-1) != 1 or x2.dtype != torch.float32:
        raise TypeError("linear: fp32 tensors with unit inner stride required")
    Wv = W if w_cols is None else W[:, w_cols[0]:w_cols[1]]
    if Wv.shape[1] != in_dim or x2.shape[1] != in_dim:
        raise ValueError(f"linear: in_dim mismatch {tuple(x2.shape)} vs {tuple(Wv.shape)}")
    out_dim = Wv.shape[0]
    rows = x2.shape[0]
    if out is None:
        out = torch.empty(*x.shape[:-1], out_dim, device=x.device, dtype=torch.float32)
    o2 = out.reshape(-1, out.shape[-1]) if out.dim() != 2 else out
    if o2.stride(-1) != 1 or o2.shape[0] != rows or o2.shape[1] < out_dim and o2.shape[1] != out_dim:
        raise ValueError("linear: bad output buffer")
    res2 = None
    if residual is not None:
        res2 = residual.reshape(-1, residual.shape[-1])
        if res2.stride(-1) != 1 or res2.shape != (rows, out_dim) or res2.dtype != torch.float32:
            raise ValueError("linear: bad residual")
    return x2, Wv, res2, out, o2


def linear(x, W, bias=None, relu=False, residual=None, out=None, w_cols=None, bn=None):
    """y = [residual +] act(x @ W[:, w_cols].T + bias), optionally followed by BatchNorm1d(eval) in the same launch
    (bn = (gamma, beta, running_mean, running_var, eps)).  x [..., in] (last dim contiguous, rows strided ok)."""
    lib = _lib.load()
    x2, Wv, res2, out, o2 = _linear_views(x, W, residual, out, w_cols)
    rows, in_dim = x2.shape
    out_dim = Wv.shape[0]
    if bias is not None:
        _chk(bias, "bias", torch.float32, (out_dim,))
    if bn is not None:
        if relu:
            raise ValueError("linear: relu and fused batch-norm are not combined")
        gamma, beta, mean, var, eps = bn
        for nm, t in (("gamma", gamma), ("beta", beta), ("running_mean", mean), ("running_var", var)):
            _chk(t, nm, torch.float32, (out_dim,))
    if rows == 0:       # an empty batch: nothing to launch (and torch hands out a null data_ptr for empty tensors)
        return out
    if bn is not None:
        _lib.check(lib.eamrl_linear_bn(_ptr(x2), x2.stride(0), _ptr(Wv), Wv.stride(0), _ptr(bias), _ptr(res2),
                                       res2.stride(0) if res2 is not None else 0, _ptr(o2), o2.stride(0), rows, in_dim,
                                       out_dim, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(var), float(eps), _stream(x)),
                   "eamrl_linear_bn")
        return out
    _lib.check(lib.eamrl_linear(_ptr(x2), x2.stride(0), _ptr(Wv), Wv.stride(0), _ptr(bias), _ptr(res2),
                                res2.stride(0) if res2 is not None else 0, _ptr(o2), o2.stride(0), rows, in_dim,
                                out_dim, int(relu), _stream(x)), "eamrl_linear")
    return out


def _matmul_right_views(x, Wt, out):
    """(x2, out, o2) of eamrl_matmul_right; `out` is allocated when None."""
    _chk(Wt, "Wt", torch.float32)
    x2 = x.reshape(-1, x.shape[-1])
    if x2.stride(-1) != 1 or x2.dtype != torch.float32:
        raise ValueError("matmul_right: bad x")
    _need_gpu(x2, "x")
    rows, in_dim = x2.shape
    if Wt.shape[0] != in_dim:
        raise ValueError("matmul_right: in_dim mismatch")
    out_dim = Wt.shape[1]
    if out is None:
        out = torch.empty(*x.shape[:-1], out_dim, device=x.device, dtype=torch.float32)
    o2 = out.reshape(-1, out.shape[-1]) if out.dim() != 2 else out
    if o2.stride(-1) != 1 or o2.shape != (rows, out_dim):
        raise ValueError("matmul_right: bad output buffer")
    return x2, out, o2


def matmul_right(x, Wt, out=None):
    """y = x @ Wt   (Wt [in][out], contiguous)."""
    lib = _lib.load()
    x2, out, o2 = _matmul_right_views(x, Wt, out)
    rows, in_dim = x2.shape
    if rows == 0:       # an empty batch: nothing to launch (and torch hands out a null data_ptr for empty tensors)
        return out
    _lib.check(lib.eamrl_matmul_right(_ptr(x2), x2.stride(0), _ptr(Wt), _ptr(o2), o2.stride(0), rows, in_dim, Wt.shape[1],
                                      _stream(x)), "eamrl_matmul_right")
    return out


def linear_variant(x, W, bias=None, relu=False, residual=None, out=None, w_cols=None, bn=None, transposed=False):
    """The EAMRL_LINEAR_* id of the kernel that linear(x, W, bias, relu, residual, out, w_cols, bn) -- or, with transposed=True,
    matmul_right(x, W, out) -- launches for these very tensors under the current debug keys (eamrl_linear_variant).  Nothing is
    launched; an `out` left to the call stands for the fresh, aligned tensor it would allocate."""
    lib = _lib.load()
    if transposed:
        if bias is not None or relu or residual is not None or w_cols is not None or bn is not None:
            raise ValueError("linear_variant: matmul_right takes x, Wt and out only")
        x2, _, o2 = _matmul_right_views(x, W, out)
        Wv, res2, ldw = W, None, W.shape[1]
    else:
        x2, Wv, res2, _, o2 = _linear_views(x, W, residual, out, w_cols)
        ldw = Wv.stride(0)
        if bn is not None and relu:
            raise ValueError("linear: relu and fused batch-norm are not combined")
    rows, in_dim = x2.shape
    out_dim = W.shape[1] if transposed else Wv.shape[0]
    if rows == 0:       # what linear / matmul_right do with an empty batch
        return _lib.LINEAR_NONE
    rc = lib.eamrl_linear_variant(_ptr(x2), x2.stride(0), _ptr(Wv), ldw, int(transposed), _ptr(bias), _ptr(res2),
                                  res2.stride(0) if res2 is not None else 0, _ptr(o2), o2.stride(0), rows, in_dim, out_dim,
                                  int(relu), int(bn is not None))
    if rc < 0:
        _lib.check(rc, "eamrl_linear_variant")
    return rc


def linear_wgrad_supported(out_dim: int, in_dim: int) -> bool:
    return _lib.load().eamrl_linear_wgrad_scratch(0, int(out_dim), int(in_dim)) >= 0


def linear_wgrad(dy, x, need_bias=True):
    """dW [out, in] = dy^T x over all rows, db [out] = column sums of dy (eamrl_linear_wgrad); dy [..., out], x [..., in]."""
    lib = _lib.load()
    dy2, x2 = dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])
    for nm, t_ in (("dy", dy2), ("x", x2)):
        _need_gpu(t_, nm)
        if t_.dtype != torch.float32 or t_.stride(-1) != 1:
            raise TypeError(f"linear_wgrad: {nm} must be fp32 with unit inner stride")
    rows, out_dim = dy2.shape
    if x2.shape[0] != rows:
        raise ValueError("linear_wgrad: row mismatch")
    in_dim = x2.shape[1]
    need = lib.eamrl_linear_wgrad_scratch(rows, out_dim, in_dim)
    if need < 0:
        raise ValueError(f"linear_wgrad: shape {out_dim} x {in_dim} not supported (multiples of 128)")
    dW = torch.empty(out_dim, in_dim, dtype=torch.float32, device=dy.device)
    db = torch.empty(out_dim, dtype=torch.float32, device=dy.device) if need_bias else None
    scratch = torch.empty(max(int(need), 4), dtype=torch.float32, device=dy.device)
    _lib.check(lib.eamrl_linear_wgrad(_ptr(dy2), dy2.stride(0), _ptr(x2), x2.stride(0), rows, out_dim, in_dim, _ptr(dW), _ptr(db),
                                      _ptr(scratch), scratch.numel(), _stream(dy)), "eamrl_linear_wgrad")
    return dW, db


def augment_xy(xy, code, cs=None, offset=0.5):
    """Coordinates [B, N, 2] -> [R, N, 2] with row r = a * B + b the instance b transformed by code[r] (eamrl_augment_xy:
    0..7 dihedral variants, 8 rotation by the angle with (cos, sin) = cs[r], 9 rotation + x <-> y)."""
    lib = _lib.load()
    _chk(xy, "xy", torch.float32)
    B, N, two = xy.shape
    if two != 2:
        raise ValueError("augment_xy: coordinates must be [B, N, 2]")
    _chk(code, "code", torch.int32)
    R = code.shape[0]
    if cs is not None:
        _chk(cs, "cs", torch.float32, (R, 2))
    out = torch.empty(R, N, 2, dtype=torch.float32, device=xy.device)
    _lib.check(lib.eamrl_augment_xy(_ptr(xy), _ptr(cs), _ptr(code), _ptr(out), R, B, N, float(offset), _stream(xy)),
               "eamrl_augment_xy")
    return out


def small_linear_wgrad(dy, x, need_bias=True):
    """dW [out, K] = dy^T x, db [out] for a Linear with K <= 8 inputs (eamrl_small_linear_wgrad); dy [..., out], x [..., K]."""
    lib = _lib.load()
    dy2, x2 = dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])
    for nm, t_ in (("dy", dy2), ("x", x2)):
        _need_gpu(t_, nm)
        if t_.dtype != torch.float32 or t_.stride(-1) != 1:
            raise TypeError(f"small_linear_wgrad: {nm} must be fp32 with unit inner stride")
    rows, out_dim = dy2.shape
    K = x2.shape[1]
    if x2.shape[0] != rows or not 1 <= K <= 8:
        raise ValueError("small_linear_wgrad: row mismatch or more than 8 input features")
    dW = torch.empty(out_dim, K, dtype=torch.float32, device=dy.device)
    db = torch.empty(out_dim, dtype=torch.float32, device=dy.device) if need_bias else None
    scratch = torch.empty(max(int(lib.eamrl_small_linear_wgrad_scratch(rows, out_dim)), 4), dtype=torch.float32, device=dy.device)
    _lib.check(lib.eamrl_small_linear_wgrad(_ptr(dy2), dy2.stride(0), _ptr(x2), x2.stride(0), rows, out_dim, K, _ptr(dW), _ptr(db),
                                            _ptr(scratch), scratch.numel(), _stream(dy)), "eamrl_small_linear_wgrad")
    return dW, db


def batchnorm_backward(x, dy, save_mean, save_var, gamma, eps, need_affine_grads=True):
    """Gradient of batchnorm_train_ (eamrl_batchnorm_backward): x = the normalisation's input [..., E] -> (dx, dgamma, dbeta)."""
    lib = _lib.load()
    _chk(x, "x", torch.float32)
    _chk(dy, "dy", torch.float32, tuple(x.shape))
    E = x.shape[-1]
    rows = x.numel() // E
    dx = torch.empty_like(x)
    dg = torch.empty(E, dtype=torch.float32, device=x.device) if need_affine_grads else None
    db = torch.empty(E, dtype=torch.float32, device=x.device) if need_affine_grads else None
    scratch = torch.empty(max(int(lib.eamrl_batchnorm_backward_scratch(rows, E)), 4), dtype=torch.float32, device=x.device)
    _lib.check(lib.eamrl_batchnorm_backward(_ptr(x), _ptr(dy), _ptr(save_mean), _ptr(save_var), _ptr(gamma), float(eps), rows, E,
                                            _ptr(dx), _ptr(dg), _ptr(db), _ptr(scratch), scratch.numel(), _stream(x)),
               "eamrl_batchnorm_backward")
    return dx, dg, db


def mha_encoder(qkv, num_heads):
    lib = _lib.load()
    _chk(qkv, "qkv", torch.float32)
    B, N, E3 = qkv.shape
    out = torch.empty(B, N, E3 // 3, device=qkv.device, dtype=torch.float32)
    _lib.check(lib.eamrl_mha_encoder(_ptr(qkv), _ptr(out), B, N, E3 // 3, num_heads, _stream(qkv)), "eamrl_mha_encoder")
    return out


def mha_encoder_backward_supported(N: int, E: int, H: int) -> bool:
    return bool(_lib.load().eamrl_mha_encoder_backward_supported(int(N), int(E), int(H)))


def mha_encoder_backward(qkv, dout, num_heads):
    """dqkv [B, N, 3E] of mha_encoder(qkv) for the output gradient dout [B, N, E] (eamrl_mha_encoder_backward)."""
    lib = _lib.load()
    _chk(qkv, "qkv", torch.float32)
    B, N, E3 = qkv.shape
    _chk(dout, "dout", torch.float32, (B, N, E3 // 3))
    dqkv = torch.empty_like(qkv)
    _lib.check(lib.eamrl_mha_encoder_backward(_ptr(qkv), _ptr(dout), _ptr(dqkv), B, N, E3 // 3, num_heads, _stream(qkv)),
               "eamrl_mha_encoder_backward")
    return dqkv


# the text of HeterogenousMHA.forward's assertion on an even graph size (zoo/ham/attention.py:69-72: a continued string literal)
ODD_NODES_MESSAGE = ("Graph size should have odd number of nodes due to pickup-delivery problem  " + " " * 37
                     + "(n/2 pickup, n/2 delivery, 1 depot)")


def hetero_mha_supported(M: int, E: int, H: int) -> bool:
    return bool(_lib.load().eamrl_hetero_mha_supported(int(M), int(E), int(H)))


def _hetero_proj_shape(proj, what):
    """(B, M, E) of a packed HAM projection [B, M, 6E] on the GPU; an even M raises the reference's assertion."""
    _chk(proj, "proj", torch.float32)
    if proj.dim() != 3 or proj.shape[2] % 6:
        raise ValueError(f"{what}: proj must be [B, M, 6E], got {tuple(proj.shape)}")
    B, M, E6 = proj.shape
    assert M % 2 == 1, ODD_NODES_MESSAGE
    return B, M, E6 // 6


def hetero_mha(proj, num_heads):
    """The heads [B, M, E] of the HAM encoder's heterogeneous attention for proj [B, M, 6E] = q | k | v | qpair | qsame |
    qother (eamrl_hetero_mha); M = 2P + 1 nodes: depot, P pickups, P deliveries."""
    lib = _lib.load()
    B, M, E = _hetero_proj_shape(proj, "hetero_mha")
    out = torch.empty(B, M, E, device=proj.device, dtype=torch.float32)
    _lib.check(lib.eamrl_hetero_mha(_ptr(proj), _ptr(out), B, M, E, num_heads, _stream(proj)), "eamrl_hetero_mha")
    return out


def hetero_mha_backward_supported(M: int, E: int, H: int) -> bool:
    return bool(_lib.load().eamrl_hetero_mha_backward_supported(int(M), int(E), int(H)))


def hetero_mha_backward(proj, dout, num_heads):
    """dproj [B, M, 6E] of hetero_mha(proj) for the output gradient dout [B, M, E] (eamrl_hetero_mha_backward)."""
    lib = _lib.load()
    B, M, E = _hetero_proj_shape(proj, "hetero_mha_backward")
    _chk(dout, "dout", torch.float32, (B, M, E))
    dproj = torch.empty_like(proj)
    _lib.check(lib.eamrl_hetero_mha_backward(_ptr(proj), _ptr(dout), _ptr(dproj), B, M, E, num_heads, _stream(proj)),
               "eamrl_hetero_mha_backward")
    return dproj


def normalize_(x, kind, gamma, beta, mean=None, var=None, eps=1e-5):
    lib = _lib.load()
    _chk(x, "x", torch.float32)
    B, N, E = x.shape
    for nm, t in (("gamma", gamma), ("beta", beta)):
        _chk(t, nm, torch.float32, (E,))
    if kind == NORM_BATCH_EVAL:
        _chk(mean, "running_mean", torch.float32, (E,))
        _chk(var, "running_var", torch.float32, (E,))
    _lib.check(lib.eamrl_normalize(_ptr(x), B, N, E, kind, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(var), eps,
                                   _stream(x)), "eamrl_normalize")
    return x


def instance_norm_forward(x, gamma, beta, eps):
    """-> (y, mean, rstd): InstanceNorm1d(affine) over the nodes of x [B, N, E], kept statistics [B, E] for the backward."""
    lib = _lib.load()
    _chk(x, "x", torch.float32)
    B, N, E = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(B, E, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B, E, dtype=torch.float32, device=x.device)
    _lib.check(lib.eamrl_instance_norm_forward(_ptr(x), _ptr(y), _ptr(mean), _ptr(rstd), B, N, E, _ptr(gamma), _ptr(beta),
                                               float(eps), _stream(x)), "eamrl_instance_norm_forward")
    return y, mean, rstd


def instance_norm_backward(x, dy, mean, rstd, gamma, need_affine_grads=True):
    """-> (dx, dgamma | None, dbeta | None)"""
    lib = _lib.load()
    _chk(x, "x", torch.float32)
    _chk(dy, "dy", torch.float32, tuple(x.shape))
    B, N, E = x.shape
    dx = torch.empty_like(x)
    dg = torch.zeros(E, dtype=torch.float32, device=x.device) if need_affine_grads else None
    db = torch.zeros(E, dtype=torch.float32, device=x.device) if need_affine_grads else None
    _lib.check(lib.eamrl_instance_norm_backward(_ptr(x), _ptr(dy), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dx), _ptr(dg),
                                                _ptr(db), B, N, E, _stream(x)), "eamrl_instance_norm_backward")
    return dx, dg, db


def batchnorm_train_(x, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """BatchNorm1d with batch statistics over all rows of x [..., E], in place; running stats updated as torch does.
    -> (x, batch_mean [E], batch_var [E] (biased))."""
    lib = _lib.load()
    _chk(x, "x", torch.float32)
    E = x.shape[-1]
    rows = x.numel() // E
    for nm, t in (("gamma", gamma), ("beta", beta)):
        _chk(t, nm, torch.float32, (E,))
    if (running_mean is None) != (running_var is None):
        raise ValueError("batchnorm_train: running_mean and running_var come together")
    if running_mean is not None:
        _chk(running_mean, "running_mean", torch.float32, (E,))
        _chk(running_var, "running_var", torch.float32, (E,))
    nws = ((rows + 127) // 128) * E
    ws = torch.empty(nws + 2 * E, device=x.device, dtype=torch.float32)
    save_mean, save_var = ws[nws:nws + E], ws[nws + E:]
    _lib.check(lib.eamrl_batchnorm_train(_ptr(x), rows, E, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                         float(momentum), float(eps), _ptr(save_mean), _ptr(save_var), _ptr(ws), nws,
                                         _stream(x)), "eamrl_batchnorm_train")
    return x, save_mean, save_var


def mean_nodes(emb):
    lib = _lib.load()
    _chk(emb, "emb", torch.float32)
    B, M, E = emb.shape
    out = torch.empty(B, E, device=emb.device, dtype=torch.float32)
    _lib.check(lib.eamrl_mean_nodes(_ptr(emb), _ptr(out), B, M, E, _stream(emb)), "eamrl_mean_nodes")
    return out


def pack_linear_weight(W, out=None):
    """torch.nn.Linear.weight [out, in] -> the packed MFMA fragment order the fused encoder reads (eamrl_pack_linear_weight)."""
    lib = _lib.load()
    _chk(W, "weight", torch.float32)
    N, K = W.shape
    if out is None:
        out = torch.empty(N * K, device=W.device, dtype=torch.float32)
    _chk(out, "packed weight", torch.float32, (N * K,))
    _lib.check(lib.eamrl_pack_linear_weight(_ptr(W), _ptr(out), N, K, _stream(W)), "eamrl_pack_linear_weight")
    return out


# the shapes eamrl_moe_ffn is built for
MOE_EMBED_DIM, MOE_HIDDEN, MOE_MAX_EXPERTS = 128, 512, 8


def moe_ffn_scratch(rows, n_exp, k) -> int:
    """Bytes of device scratch `moe_ffn` needs (eamrl_moe_ffn_scratch; host only): 64 + 16 * ceil(rows * n_exp / 4) +
    512 * rows * k, or -1 for a shape outside 1 <= k <= n_exp <= 8."""
    return int(_lib.load().eamrl_moe_ffn_scratch(int(rows), int(n_exp), int(k)))


def pack_moe_experts(W1, b1, W2, b2, out=None):
    """The experts' parameters -- lists of n_exp tensors W1 [512, 128], b1 [512], W2 [128, 512], b2 [128] -- as the operand dict of
    `moe_ffn`: W1p / W2p [n_exp, 65536] in the fragment order of `pack_linear_weight`, b1 [n_exp, 512], b2 [n_exp, 128].
    out: such a dict to refresh in place (a captured graph keeps reading its buffers)."""
    n = len(W1)
    dev = W1[0].device
    if out is None:
        out = {"W1p": torch.empty(n, MOE_HIDDEN * MOE_EMBED_DIM, device=dev), "b1": torch.empty(n, MOE_HIDDEN, device=dev),
               "W2p": torch.empty(n, MOE_EMBED_DIM * MOE_HIDDEN, device=dev), "b2": torch.empty(n, MOE_EMBED_DIM, device=dev)}
    for e in range(n):
        _chk(W1[e], "expert lins.0.weight", torch.float32, (MOE_HIDDEN, MOE_EMBED_DIM))
        _chk(W2[e], "expert lins.1.weight", torch.float32, (MOE_EMBED_DIM, MOE_HIDDEN))
        pack_linear_weight(W1[e], out=out["W1p"][e])
        pack_linear_weight(W2[e], out=out["W2p"][e])
        out["b1"][e].copy_(b1[e])
        out["b2"][e].copy_(b2[e])
    return out


_MOE_SCRATCH = {}


def _moe_scratch(device, need):
    """The scratch of `moe_ffn`, kept per (device, stream) and grown on demand: the calls of one stream run one after the
    other, so the layers of an encoder share it (106 MB at 103 424 rows, k = 2).  Under HIP-graph capture a private buffer is
    allocated instead, in the graph's own pool."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(need, device=device, dtype=torch.uint8)
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = _MOE_SCRATCH.get(key)
    if buf is None or buf.numel() < need:
        _MOE_SCRATCH[key] = buf = torch.empty(need, device=device, dtype=torch.uint8)
    return buf


def moe_ffn(x, w_gate, experts, k, w_noise=None, noise=None, residual=None, bn=None, out=None, return_routing=False):
    """[BN_eval](residual + MoE(x)) for x [..., 128]: noisy top-k gating over n_exp = w_gate.shape[1] experts, the selected
    experts' 128 -> 512 -> 128 ReLU MLPs and their gate-weighted sum (eamrl_moe_ffn: three launches, no host synchronisation).
    experts: the dict of `pack_moe_experts`.  noise [rows, n_exp] standard-normal draws (with w_noise): training-mode noisy
    gating; None: clean logits.  bn = (gamma, beta, running_mean, running_var, eps).  out may be `residual` (in place).
    return_routing: also (sel [rows, k] int8, gates [rows, k]), larger gate first."""
    lib = _lib.load()
    _chk(x, "x", torch.float32)
    _chk(w_gate, "w_gate", torch.float32)
    E, n_exp, k = x.shape[-1], w_gate.shape[1] if w_gate.dim() == 2 else -1, int(k)
    rows = x.numel() // max(E, 1)
    if E != MOE_EMBED_DIM or w_gate.dim() != 2 or w_gate.shape[0] != E:
        raise NotImplementedError(f"moe_ffn: embed_dim {E} with w_gate {tuple(w_gate.shape)}; the kernels are built for embed_dim "
                                  f"{MOE_EMBED_DIM} and w_gate [{MOE_EMBED_DIM}, n_exp]")
    if not 1 <= k <= n_exp <= MOE_MAX_EXPERTS:
        raise NotImplementedError(f"moe_ffn: k = {k}, num_experts = {n_exp}; built for 1 <= k <= num_experts <= {MOE_MAX_EXPERTS}")
    _chk(experts["W1p"], "experts['W1p']", torch.float32, (n_exp, MOE_HIDDEN * E))
    _chk(experts["b1"], "experts['b1']", torch.float32, (n_exp, MOE_HIDDEN))
    _chk(experts["W2p"], "experts['W2p']", torch.float32, (n_exp, E * MOE_HIDDEN))
    _chk(experts["b2"], "experts['b2']", torch.float32, (n_exp, E))
    if noise is not None:
        if w_noise is None:
            raise ValueError("moe_ffn: noise needs w_noise")
        _chk(w_noise, "w_noise", torch.float32, (E, n_exp))
        _chk(noise, "noise", torch.float32, (rows, n_exp))
    if residual is not None:
        _chk(residual, "residual", torch.float32, tuple(x.shape))
    if out is None:
        out = torch.empty_like(x)
    _chk(out, "out", torch.float32, tuple(x.shape))
    m = _lib.MoeLayer()
    if bn is not None:
        gamma, beta, mean, var, eps = bn
        for nm, t in (("gamma", gamma), ("beta", beta), ("running_mean", mean), ("running_var", var)):
            _chk(t, nm, torch.float32, (E,))
        m.bn_gamma, m.bn_beta, m.bn_mean, m.bn_var, m.bn_eps = gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(), float(eps)
    sel = torch.empty(rows, k, device=x.device, dtype=torch.int8)
    g = torch.empty(rows, k, device=x.device, dtype=torch.float32)
    if rows == 0:
        return (out, sel, g) if return_routing else out
    need = lib.eamrl_moe_ffn_scratch(rows, n_exp, k)
    if need < 0:
        raise NotImplementedError(f"moe_ffn: {rows} rows are above the 2^24 rows of one call")
    scratch = _moe_scratch(x.device, need)
    m.x, m.w_gate = x.data_ptr(), w_gate.data_ptr()
    if noise is not None:
        m.w_noise, m.noise = w_noise.data_ptr(), noise.data_ptr()
    m.W1p, m.b1, m.W2p, m.b2 = (experts[n].data_ptr() for n in ("W1p", "b1", "W2p", "b2"))
    if residual is not None:
        m.res = residual.data_ptr()
    m.y, m.sel, m.g, m.scratch, m.scratch_bytes = out.data_ptr(), sel.data_ptr(), g.data_ptr(), scratch.data_ptr(), need
    m.rows, m.embed_dim, m.hidden, m.n_exp, m.k = rows, E, MOE_HIDDEN, n_exp, k
    _lib.check(lib.eamrl_moe_ffn(C.byref(m), _stream(x)), "eamrl_moe_ffn")
    return (out, sel, g) if return_routing else out


def moe_experts_forward_scratch(rows, n_exp, k) -> int:
    """Bytes of the state `moe_experts_forward` leaves for the backward (eamrl_moe_experts_forward_scratch; host only):
    64 + 16 * ceil(rows * n_exp / 4) + 512 * rows * k + 16 * ceil(rows * k / 16) + 32 * ceil(rows / 256), or -1."""
    return int(_lib.load().eamrl_moe_experts_forward_scratch(int(rows), int(n_exp), int(k)))


def moe_experts_backward_scratch(rows, n_exp, k) -> int:
    """Bytes of device scratch `moe_experts_backward` needs (eamrl_moe_experts_backward_scratch; host only):
    5632 * rows * k + 264192 * n_exp * max(1, min(128 // n_exp, ceil(rows * k / 64))), or -1."""
    return int(_lib.load().eamrl_moe_experts_backward_scratch(int(rows), int(n_exp), int(k)))


def pack_moe_experts_backward(W1, W2, out=None):
    """The packs of the experts' backward next to those of `pack_moe_experts`: W1Tp [n_exp, 65536] = pack_linear_weight of
    W1^T [128, 512] (dx = dHid W1), W2Tp [n_exp, 65536] = of W2^T [512, 128] (dHid = dO W2).  out: such a dict to refresh."""
    n = len(W1)
    dev = W1[0].device
    if out is None:
        out = {"W1Tp": torch.empty(n, MOE_EMBED_DIM * MOE_HIDDEN, device=dev), "W2Tp": torch.empty(n, MOE_HIDDEN * MOE_EMBED_DIM, device=dev)}
    for e in range(n):
        _chk(W1[e], "expert lins.0.weight", torch.float32, (MOE_HIDDEN, MOE_EMBED_DIM))
        _chk(W2[e], "expert lins.1.weight", torch.float32, (MOE_EMBED_DIM, MOE_HIDDEN))
        pack_linear_weight(W1[e].t().contiguous(), out=out["W1Tp"][e])
        pack_linear_weight(W2[e].t().contiguous(), out=out["W2Tp"][e])
    return out


def _moe_experts_struct(what, x, g, experts, names):
    """(struct, rows, n_exp, k) of eamrl_moe_experts with x, g and the packs `names` of `experts` checked and bound."""
    _chk(x, "x", torch.float32)
    _chk(g, "gates", torch.float32)
    E = x.shape[-1]
    rows = x.numel() // max(E, 1)
    if E != MOE_EMBED_DIM:
        raise NotImplementedError(f"{what}: embed_dim {E}; the kernels are built for embed_dim {MOE_EMBED_DIM}")
    n_exp = experts["b1"].shape[0] if isinstance(experts.get("b1"), torch.Tensor) and experts["b1"].dim() == 2 else -1
    k = g.shape[1] if g.dim() == 2 else -1
    if not 1 <= k <= n_exp <= MOE_MAX_EXPERTS:
        raise NotImplementedError(f"{what}: k = {k}, num_experts = {n_exp}; built for 1 <= k <= num_experts <= {MOE_MAX_EXPERTS}")
    _chk(g, "gates", torch.float32, (rows, k))
    shapes = {"W1p": (n_exp, MOE_HIDDEN * E), "b1": (n_exp, MOE_HIDDEN), "W2p": (n_exp, E * MOE_HIDDEN), "b2": (n_exp, E),
              "W1Tp": (n_exp, E * MOE_HIDDEN), "W2Tp": (n_exp, MOE_HIDDEN * E)}
    m = _lib.MoeExperts()
    for nm in names:
        setattr(m, nm, _chk(experts[nm], f"experts['{nm}']", torch.float32, shapes[nm]).data_ptr())
    m.x, m.g = x.data_ptr(), g.data_ptr()
    m.rows, m.embed_dim, m.hidden, m.n_exp, m.k = rows, E, MOE_HIDDEN, n_exp, k
    return m, rows, n_exp, k


def moe_experts_forward(x, sel, g, experts):
    """The selected experts on a GIVEN routing (eamrl_moe_experts_forward): y[row] = sum over the row's slots, in ascending
    expert index sel[row, j], of g[row, j] * expert(x[row]) -- with the (sel, g) `moe_ffn` returned, `moe_ffn`'s y bit for bit.
    x [..., 128]; sel [rows, k] int8; g [rows, k]; experts: the dict of `pack_moe_experts`.  Returns (y, state): `state` (a
    uint8 tensor: row counts and row lists in ascending row order, per-slot expert outputs, the checked routing) is what
    `moe_experts_backward` reads.  A `sel` entry outside 0 .. n_exp - 1 or repeated within its row is dropped on the device
    (no contribution, zero gate gradient) and counted: `moe_experts_dropped(state)`."""
    lib = _lib.load()
    _chk(x, "x", torch.float32)
    m, rows, n_exp, k = _moe_experts_struct("moe_experts_forward", x, g, experts, ("W1p", "b1", "W2p", "b2"))
    _chk(sel, "sel", torch.int8, (rows, k))
    y = torch.empty_like(x)
    need = lib.eamrl_moe_experts_forward_scratch(rows, n_exp, k)
    if need < 0:
        raise NotImplementedError(f"moe_experts_forward: {rows} rows are above the 2^24 rows of one call")
    state = torch.empty(need, device=x.device, dtype=torch.uint8)
    if rows == 0:
        return y, state
    m.sel, m.y, m.state, m.state_bytes = sel.data_ptr(), y.data_ptr(), state.data_ptr(), need
    _lib.check(lib.eamrl_moe_experts_forward(C.byref(m), _stream(x)), "eamrl_moe_experts_forward")
    return y, state


def moe_experts_dropped(state) -> int:
    """How many `sel` entries the forward that wrote `state` dropped (counter word 15; synchronises with the host)."""
    return int(state[60:64].view(torch.int32).item()) if state.numel() >= 64 else 0


def moe_experts_backward(dy, x, g, experts, state, need_dx=True, need_dg=True, need_weight_grads=True):
    """Backward of `moe_experts_forward` (eamrl_moe_experts_backward) from dy [..., 128] and the forward's x, g, `state`:
    -> (dx like x, dg [rows, k], dW1 [n_exp, 512, 128], db1 [n_exp, 512], dW2 [n_exp, 128, 512], db2 [n_exp, 128]); the ones not
    asked for are None.  experts: the dicts of `pack_moe_experts` and `pack_moe_experts_backward` merged (W1p, b1, W1Tp, W2Tp are
    read).  An expert without rows gets zero gradients; two calls on the same inputs give the same bits."""
    lib = _lib.load()
    _chk(dy, "dy", torch.float32, tuple(x.shape))
    m, rows, n_exp, k = _moe_experts_struct("moe_experts_backward", x, g, experts, ("W1p", "b1", "W1Tp", "W2Tp"))
    need_state = lib.eamrl_moe_experts_forward_scratch(rows, n_exp, k)
    need = lib.eamrl_moe_experts_backward_scratch(rows, n_exp, k)
    if need < 0:
        raise NotImplementedError(f"moe_experts_backward: {rows} rows are above the 2^24 rows of one call")
    _chk(state, "state", torch.uint8, (need_state,))
    dev = x.device
    dx = torch.empty_like(x) if need_dx else None
    dg = torch.empty(rows, k, device=dev, dtype=torch.float32) if need_dg else None
    dW1 = db1 = dW2 = db2 = None
    if need_weight_grads:
        dW1, db1 = torch.empty(n_exp, MOE_HIDDEN, MOE_EMBED_DIM, device=dev), torch.empty(n_exp, MOE_HIDDEN, device=dev)
        dW2, db2 = torch.empty(n_exp, MOE_EMBED_DIM, MOE_HIDDEN, device=dev), torch.empty(n_exp, MOE_EMBED_DIM, device=dev)
    if rows == 0:
        for t in (dW1, db1, dW2, db2):
            if t is not None:
                t.zero_()
        return dx, dg, dW1, db1, dW2, db2
    scratch = _moe_scratch(dev, need)
    m.dy, m.state, m.state_bytes, m.scratch, m.scratch_bytes = dy.data_ptr(), state.data_ptr(), need_state, scratch.data_ptr(), need
    for nm, t in (("dx", dx), ("dg", dg), ("dW1", dW1), ("db1", db1), ("dW2", dW2), ("db2", db2)):
        if t is not None:
            setattr(m, nm, t.data_ptr())
    _lib.check(lib.eamrl_moe_experts_backward(C.byref(m), _stream(x)), "eamrl_moe_experts_backward")
    return dx, dg, dW1, db1, dW2, db2


def encoder_fused_supported(M, E, H, ff_hidden, nlayers) -> bool:
    return bool(_lib.load().eamrl_encoder_fused_supported(int(M), int(E), int(H), int(ff_hidden), int(nlayers)))


def encoder_fused(h, layers, num_heads, ff_hidden, norm, eps, cache=None, init=None, store_hidden=True):
    """All encoder layers of every instance in one launch.  h [B, M, E]; layers: list of dicts with the 16 fields of
    struct eamrl_encoder_layer (packed weights, biases, norm parameters; running stats may be None for instance norm).
    cache = (Wc_packed, WoutT_packed, out [B, M, ld], nproj[, Wg [E, E], gctx [B, E]]): also fill the slot-major decoder
    cache and, with the last two, the graph context (struct eamrl_encoder_cache).
    init (instead of h; struct eamrl_encoder_init) = dict(feat [B, M, F], W [E, F], b, depot [B, >= 2] or None, Wd, bd,
    want_init): the init embedding is computed inside the kernel; returns (hidden or None, init embeddings or None) then.
    store_hidden=False (with init and cache): the node embeddings never leave LDS."""
    return _encoder_fused_call(h, layers, num_heads, ff_hidden, norm, eps, cache, init, store_hidden, None)


# packed 16-bit weights: the torch dtype of the buffer names the operand type of the kernel
DTYPE16 = {torch.float16: 1, torch.bfloat16: 2}      # EAMRL_DTYPE_F16, EAMRL_DTYPE_BF16


def pack_linear_weight16(W, dtype, out=None):
    """torch.nn.Linear.weight [out, in] (fp32) -> rounded to `dtype` (torch.float16 / torch.bfloat16, round to nearest
    even) in the 16-bit MFMA fragment order of the 16-bit fused encoder (eamrl_pack_linear_weight16)."""
    lib = _lib.load()
    if dtype not in DTYPE16:
        raise ValueError(f"pack_linear_weight16: dtype must be torch.float16 or torch.bfloat16, got {dtype}")
    _chk(W, "weight", torch.float32)
    N, K = W.shape
    if N % 16 or K % 32:
        raise ValueError("pack_linear_weight16: out_dim must be a multiple of 16 and in_dim of 32")
    if out is None:
        out = torch.empty(N * K, device=W.device, dtype=dtype)
    _chk(out, "packed weight", dtype, (N * K,))
    _lib.check(lib.eamrl_pack_linear_weight16(_ptr(W), _ptr(out), N, K, DTYPE16[dtype], _stream(W)), "eamrl_pack_linear_weight16")
    return out


def encoder_fused16_supported(M, E, H, ff_hidden, nlayers, dtype=torch.bfloat16) -> bool:
    if dtype not in DTYPE16:
        return False
    return bool(_lib.load().eamrl_encoder_fused16_supported(int(M), int(E), int(H), int(ff_hidden), int(nlayers), DTYPE16[dtype]))


def encoder_fused16(h, layers, num_heads, ff_hidden, norm, eps, dtype, cache=None, init=None, store_hidden=True):
    """`encoder_fused` with 16-bit MFMA operands ("16-bit encoder"): the weights Wqkv / Wo / W1 / W2 of every
    layer and the cache's Wc / WoutT are `pack_linear_weight16` buffers of `dtype` (torch.float16 / torch.bfloat16); all
    other arguments, the inputs and the outputs are fp32 and as for `encoder_fused`.  No autograd."""
    if dtype not in DTYPE16:
        raise ValueError(f"encoder_fused16: dtype must be torch.float16 or torch.bfloat16, got {dtype}")
    return _encoder_fused_call(h, layers, num_heads, ff_hidden, norm, eps, cache, init, store_hidden, dtype)


_PACKED_FIELDS = ("Wqkv", "Wo", "W1", "W2")


def _encoder_fused_call(h, layers, num_heads, ff_hidden, norm, eps, cache, init, store_hidden, dtype):
    """encoder_fused (dtype None) / encoder_fused16 (dtype = the packed weights' torch dtype)."""
    what = "encoder_fused" if dtype is None else "encoder_fused16"
    wdt = torch.float32 if dtype is None else dtype
    lib = _lib.load()
    if init is not None:
        feat = init["feat"]
        _chk(feat, "node features", torch.float32)
        B, M, F = feat.shape
        W = init["W"]
        E = W.shape[0]
        _chk(W, "init_embed.weight", torch.float32, (E, F))
        dev = feat.device
    else:
        _chk(h, "h", torch.float32)
        B, M, E = h.shape
        dev = h.device
    arr = (_lib.EncoderLayer * len(layers))()
    for i, d in enumerate(layers):
        for name, _ in _lib.EncoderLayer._fields_:
            t = d.get(name)
            if t is not None:
                _need_gpu(t, name)
                want = wdt if name in _PACKED_FIELDS else torch.float32
                if t.dtype != want or not t.is_contiguous():
                    raise TypeError(f"{what}: {name} must be contiguous {want}")
            setattr(arr[i], name, _ptr(t))
    out = torch.empty(B, M, E, dtype=torch.float32, device=dev) if (store_hidden or cache is None) else None
    cstruct = None
    if cache is not None:
        Wc, WoT, buf, nproj = cache[:4]
        Wg, gctx = cache[4:6] if len(cache) >= 6 else (None, None)
        _chk(Wc, "packed cache weights", wdt, (nproj * E * E,))
        _chk(WoT, "packed project_out^T", wdt, (E * E,))
        _chk(buf, "decoder cache", torch.float32)
        if buf.dim() != 3 or buf.shape[0] != B or buf.shape[1] != M or buf.shape[2] < (nproj + 1) * E:
            raise ValueError(f"{what}: cache buffer must be [B, M, >= (nproj + 1) * E]")
        cs = _lib.EncoderCache()
        cs.Wc, cs.WoutT, cs.out, cs.ld, cs.nproj = _ptr(Wc), _ptr(WoT), _ptr(buf), buf.shape[2], int(nproj)
        if Wg is not None:
            _chk(Wg, "project_fixed_context.weight", torch.float32, (E, E))
            _chk(gctx, "graph context", torch.float32, (B, E))
            if Wg.data_ptr() % 16:
                raise ValueError(f"{what}: Wg must be 16-byte aligned")
            cs.Wg, cs.gctx = _ptr(Wg), _ptr(gctx)
        cstruct = C.byref(cs)
    if init is not None:
        ist = _lib.EncoderInit()
        b, depot, Wd, bd = init.get("b"), init.get("depot"), init.get("Wd"), init.get("bd")
        for name, t in (("init_embed.bias", b), ("depot", depot), ("init_embed_depot.weight", Wd), ("init_embed_depot.bias", bd)):
            if t is not None:
                _need_gpu(t, name)
                if t.dtype != torch.float32:
                    raise TypeError(f"{what}: {name} must be fp32")
        if depot is not None and (depot.dim() != 2 or depot.stride(1) != 1 or depot.shape[0] != B or Wd is None or not Wd.is_contiguous()):
            raise ValueError(f"{what}: depot must be [B, >= 2] with unit inner stride, Wd [E, 2] contiguous")
        init_out = torch.empty(B, M, E, dtype=torch.float32, device=dev) if init.get("want_init") else None
        ist.feat, ist.F, ist.W, ist.b = _ptr(feat), int(F), _ptr(W), _ptr(b)
        ist.depot, ist.depot_ld = _ptr(depot), (depot.stride(0) if depot is not None else 0)
        ist.Wd, ist.bd, ist.init_out = _ptr(Wd), _ptr(bd), _ptr(init_out)
        if dtype is None:
            _lib.check(lib.eamrl_encoder_fused_init(C.byref(ist), _ptr(out), B, M, E, int(num_heads), int(ff_hidden), len(layers),
                                                    int(norm), float(eps), C.cast(arr, C.c_void_p), cstruct, _stream(feat)),
                       "eamrl_encoder_fused_init")
        else:
            _lib.check(lib.eamrl_encoder_fused16_init(C.byref(ist), _ptr(out), B, M, E, int(num_heads), int(ff_hidden),
                                                      len(layers), int(norm), float(eps), C.cast(arr, C.c_void_p), cstruct,
                                                      DTYPE16[dtype], _stream(feat)), "eamrl_encoder_fused16_init")
        return out, init_out
    if dtype is None:
        _lib.check(lib.eamrl_encoder_fused(_ptr(h), _ptr(out), B, M, E, int(num_heads), int(ff_hidden), len(layers), int(norm),
                                           float(eps), C.cast(arr, C.c_void_p), cstruct, _stream(h)), "eamrl_encoder_fused")
    else:
        _lib.check(lib.eamrl_encoder_fused16(_ptr(h), _ptr(out), B, M, E, int(num_heads), int(ff_hidden), len(layers), int(norm),
                                             float(eps), C.cast(arr, C.c_void_p), cstruct, DTYPE16[dtype], _stream(h)),
                   "eamrl_encoder_fused16")
    return out


def pointer_attention(query, key, value, logit_key, attn_mask, Wout, bout=None, num_heads=8, mask_inner=True):
    """PointerAttention.forward (nn/attention.py:282-306) in one launch.  query [B, L, E] (or [B, E]); key / value /
    logit_key [B, M, E] (views with a common row stride are fine, e.g. the chunks of one projection);
    attn_mask [B, M] or [B, L, M] bool (True = feasible) or None.  -> logits [B, L, M] ([B, M] when L == 1, as the
    reference's `.squeeze(-2)` gives)."""
    lib = _lib.load()
    if query.dim() == 2:
        query = query[:, None, :]
    _chk(query, "query", torch.float32)
    B, L, E = query.shape
    M = key.shape[-2]
    ld = key.stride(-2)
    for nm, t in (("key", key), ("value", value), ("logit_key", logit_key)):
        _need_gpu(t, nm)
        if (t.dtype != torch.float32 or t.dim() != 3 or tuple(t.shape) != (B, M, E) or t.stride(-1) != 1 or t.stride(-2) != ld
                or t.stride(0) != M * ld):
            raise ValueError(f"pointer_attention: {nm} must be fp32 [B, M, E] with unit inner stride and a common row stride")
    _chk(Wout, "project_out.weight", torch.float32, (E, E))
    if bout is not None:
        _chk(bout, "project_out.bias", torch.float32, (E,))
    per_query = 0
    if attn_mask is not None:
        per_query = int(attn_mask.dim() == 3)
        _chk(attn_mask, "attn_mask", torch.bool, (B, L, M) if per_query else (B, M))
    out = torch.empty(B, L, M, device=query.device, dtype=torch.float32)
    _lib.check(lib.eamrl_pointer_attention(_ptr(query), _ptr(key), _ptr(value), _ptr(logit_key), ld,
                                           _ptr(None if attn_mask is None else _bytes(attn_mask)), per_query, _ptr(Wout),
                                           _ptr(bout), _ptr(out), B, L, M, E, int(num_heads), int(bool(mask_inner)),
                                           _stream(query)), "eamrl_pointer_attention")
    return out.squeeze(-2) if L == 1 else out


# ------------------------------------------------------------------------------------------------------
# teacher-forced re-evaluation (training gradient path)
# ------------------------------------------------------------------------------------------------------
def reeval_supported(M, E, H) -> bool:
    return bool(_lib.load().eamrl_reeval_supported(int(M), int(E), int(H)))


def pack_mask_bits_(mask, bits, t):
    """bits[:, t] <- the bit set of mask [R, M] (bool / uint8); bits [R, T, 4] int32."""
    lib = _lib.load()
    R, M = mask.shape
    _chk(_bytes(mask), "action_mask", torch.uint8, (R, M))
    _chk(bits, "mask bits", torch.int32)
    if bits.dim() != 3 or bits.shape[0] != R or bits.shape[2] != 4:
        raise ValueError("pack_mask_bits: bits must be [R, T, 4] int32")
    _lib.check(lib.eamrl_pack_mask_bits(_ptr(_bytes(mask)), _ptr(bits), R, M, bits.shape[1], int(t), _stream(mask)),
               "eamrl_pack_mask_bits")


def replay_states(st, actions, B):
    """Depot envs (cvrp, cvrptw, pctsp, op): mask bits [R, T, 4], current node idxA [R, T] and the state scalars
    sc [NC, R, T] BEFORE every step of actions [R, T], starting from the flat state `st` (not modified) -- one launch
    (eamrl_replay_states) instead of T rounds of pack-bits / copy / step."""
    lib = _lib.load()
    _chk(actions, "actions", torch.int64)
    R, T = actions.shape
    if R != st.R or st.env_name not in ("cvrp", "cvrptw", "pctsp", "op") or st.M > 1024:
        raise ValueError("replay_states: cvrp / cvrptw / pctsp / op states of at most 1024 nodes, one action row per state row")
    dev = actions.device
    NC = env_spec.ENV_SPECS[st.env_name].n_state_cols
    # (graphs above 112 nodes: the chunked layout of the key-chunked re-evaluation kernels)
    bits = torch.empty((R, T, -(-st.M // 112), 4) if st.M > 112 else (R, T, 4), dtype=torch.int32, device=dev)
    idxA = torch.empty(R, T, dtype=torch.int32, device=dev)
    sc = torch.empty(NC, R, T, dtype=torch.float32, device=dev)
    ss = st.struct()
    _lib.check(lib.eamrl_replay_states(ENVS[st.env_name], C.byref(ss), R, int(B), st.M, _ptr(actions), T, _ptr(bits), _ptr(idxA),
                                       _ptr(sc), _stream(actions)), "eamrl_replay_states")
    return bits, idxA, sc


KEY_CHUNK = 112        # keys per chunk of the re-evaluation kernels (graphs above 112 nodes: csrc/reeval.hip)


def tsp_mask_bits_chunked(actions, M):
    """TSP masks of every step in the layout of the key-chunked re-evaluation: int32 [R, T, nkc, 4], bit i of chunk c = node 112 c + i."""
    lib = _lib.load()
    _chk(actions, "actions", torch.int64)
    R, T = actions.shape
    nkc = -(-int(M) // KEY_CHUNK)
    bits = torch.empty(R, T, nkc, 4, dtype=torch.int32, device=actions.device)
    _lib.check(lib.eamrl_tsp_mask_bits_chunked(_ptr(actions), _ptr(bits), R, int(M), T, _stream(actions)), "eamrl_tsp_mask_bits_chunked")
    return bits


def pack_mask_bits_chunked_(mask, bits, t):
    """bits[:, t] (int32 [R, T, nkc, 4], chunked layout) <- mask [R, M] (bool / uint8)."""
    lib = _lib.load()
    R, M = mask.shape
    _chk(bits, "mask bits", torch.int32)
    nkc = -(-int(M) // KEY_CHUNK)
    if bits.dim() != 4 or bits.shape[0] != R or bits.shape[2] != nkc or bits.shape[3] != 4:
        raise ValueError("pack_mask_bits_chunked: bits must be [R, T, nkc, 4] int32")
    _lib.check(lib.eamrl_pack_mask_bits_chunked(_ptr(_bytes(mask)), _ptr(bits), R, M, bits.shape[1], int(t), _stream(mask)),
               "eamrl_pack_mask_bits_chunked")


def replay_states_sdvrp(st, actions):
    """SDVRP: as replay_states, plus the remaining demands rem [R, T, 128] (zero padded rows) before every step -- what the
    dynamic embedding multiplies (eamrl_replay_states_sdvrp)."""
    lib = _lib.load()
    _chk(actions, "actions", torch.int64)
    R, T = actions.shape
    if R != st.R or st.env_name != "sdvrp" or st.M > 1024:
        raise ValueError("replay_states_sdvrp: an sdvrp state of at most 1024 nodes, one action row per state row")
    dev = actions.device
    big = st.M > KEY_CHUNK             # the chunked layout of the key-chunked re-evaluation kernels
    nkc = -(-st.M // KEY_CHUNK)
    bits = torch.empty((R, T, nkc, 4) if big else (R, T, 4), dtype=torch.int32, device=dev)
    idxA = torch.empty(R, T, dtype=torch.int32, device=dev)
    sc = torch.empty(1, R, T, dtype=torch.float32, device=dev)
    rem = torch.zeros(R, T, nkc, 128, dtype=torch.float32, device=dev) if big else torch.empty(R, T, 128, dtype=torch.float32, device=dev)
    ss = st.struct()
    _lib.check(lib.eamrl_replay_states_sdvrp(C.byref(ss), R, st.M, _ptr(actions), T, _ptr(bits), _ptr(idxA), _ptr(sc), _ptr(rem),
                                             _stream(actions)), "eamrl_replay_states_sdvrp")
    return bits, idxA, sc, rem


def tsp_mask_bits(actions, M):
    lib = _lib.load()
    _chk(actions, "actions", torch.int64)
    R, T = actions.shape
    bits = torch.empty(R, T, 4, dtype=torch.int32, device=actions.device)
    _lib.check(lib.eamrl_tsp_mask_bits(_ptr(actions), _ptr(bits), R, int(M), T, _stream(actions)), "eamrl_tsp_mask_bits")
    return bits


class ReevalPlan:
    """Arguments of eamrl_reeval_forward / _backward (struct eamrl_reeval) kept alive between the two calls.

    buf [B, M, P*E]: the instance operands side by side -- K | V | Lp | Pa (| Pb); gctx [B, E] or None; cvec [NC, E] or
    None; idxA / idxB int32 [R, T]; sc [NC, R, T]; maskbits int32 [R, T, 4]; actions int64 [R, T]."""

    def __init__(self, buf, has_pb, gctx, cvec, idxA, idxB, sc, maskbits, actions, S, tstart, clip, temp, rollout_logp=None,
                 slots=None, E=None, want_entropy=False, rollout_heads=None, rem=None, dyn=None):
        _chk(buf, "operands", torch.float32)
        # slots: {"K", "V", "Lp", "Pa"[, "Pb"]} -> E-wide column block of buf (default: side by side in that order); with it
        # the plan reads a decoder cache (ops.DecodeCache.buf) in place
        # (a decoder cache of a large graph keeps its operands as planes [P, B, M, E] instead of side by side [B, M, P * E])
        self.planes = buf.dim() == 4
        if self.planes:
            _, self.B, self.M, width = buf.shape
            E = width
        else:
            self.B, self.M, width = buf.shape
        self.slots = slots or {n: i for i, n in enumerate(["K", "V", "Lp", "Pa"] + (["Pb"] if has_pb else []))}
        self.E = E if E is not None else width // (5 if has_pb else 4)
        self.buf, self.has_pb, self.gctx, self.cvec = buf, has_pb, gctx, cvec
        self.entropy = self.lse_ent = None
        self.want_entropy = bool(want_entropy)
        R, T = actions.shape
        if R != S * self.B:
            raise ValueError("reeval: rows must be S * B")
        _chk(actions, "actions", torch.int64, (R, T))
        _chk(idxA, "idxA", torch.int32, (R, T))
        if has_pb:
            _chk(idxB, "idxB", torch.int32, (R, T))
        # graphs above 112 nodes: key chunks (csrc/reeval.hip) -- chunked mask layout, a scratch that lives from forward to backward,
        # the forward pass always runs (its statistics feed the backward), no rollout heads
        self.nkc = -(-self.M // KEY_CHUNK) if self.M > KEY_CHUNK else 1
        self.scratch = None
        if self.nkc > 1:
            _chk(maskbits, "mask bits", torch.int32, (R, T, self.nkc, 4))
            rollout_heads = None
        else:
            _chk(maskbits, "mask bits", torch.int32, (R, T, 4))
        self.NC = 0 if cvec is None else cvec.shape[0]
        if self.NC:
            _chk(cvec, "state columns", torch.float32, (self.NC, self.E))
            _chk(sc, "state scalars", torch.float32, (self.NC, R, T))
        if gctx is not None:
            _chk(gctx, "graph context", torch.float32, (self.B, self.E))
        self.idxA, self.idxB, self.sc, self.maskbits, self.actions = idxA, idxB, sc, maskbits, actions
        self.R, self.T, self.S, self.tstart, self.clip, self.temp = R, T, int(S), int(tstart), float(clip), float(temp)
        self.nchunk = max(1, min(self.S, -(-512 // self.B)))
        # rollout_logp [R, T]: the per-step log-probs the rollout kernel produced for exactly these actions.  Then no
        # forward pass is needed for the gradient: forward() hands them back and the backward recovers the normaliser.
        # rollout_heads [R, Th, E]: every decode step's glimpse output as the rollout kernel computed it (RolloutState.heads):
        # the backward reads them instead of recomputing the glimpse (row r, step t at [r, t - tstart])
        # SDVRP: rem [R, T, 128] remaining demands per (row, step), dyn [3, E] = wk | wv | lw of the dynamic embedding
        self.rem = self.dyn = None
        if dyn is not None:
            _chk(rem, "remaining demands", torch.float32, (R, T, 128) if self.M <= KEY_CHUNK else (R, T, -(-self.M // KEY_CHUNK), 128))
            _chk(dyn, "dynamic embedding vectors", torch.float32, (3, self.E))
            self.rem, self.dyn = rem, dyn
            rollout_heads = None        # (the kernels recompute the glimpse for this env)
        self.heads = None
        if rollout_heads is not None:
            _chk(rollout_heads, "rollout heads", torch.float32)
            if rollout_heads.dim() != 3 or rollout_heads.shape[0] != R or rollout_heads.shape[2] != self.E \
                    or rollout_heads.shape[1] < T - int(tstart):
                raise ValueError("reeval: rollout heads must be [R, >= T - tstart, E]")
            self.heads = rollout_heads
        if rollout_logp is not None and self.nkc == 1:
            _chk(rollout_logp, "rollout log-probs", torch.float32, (R, T))
            self.logp, self.lse = rollout_logp, None
        else:
            self.logp = torch.empty(R, T, dtype=torch.float32, device=buf.device)
            self.lse = torch.empty(R, T, dtype=torch.float32, device=buf.device)

    def _struct(self):
        s = _lib.Reeval()
        E4 = self.B * self.M * self.E * 4 if self.planes else self.E * 4
        base = self.buf.data_ptr()
        s.K, s.V, s.Lp, s.Pa = (C.c_void_p(base + self.slots[n] * E4) for n in ("K", "V", "Lp", "Pa"))
        s.Pb = C.c_void_p(base + self.slots["Pb"] * E4) if self.has_pb else None
        s.ld = self.buf.shape[-1]
        s.gctx, s.Cvec, s.NC = _ptr(self.gctx), _ptr(self.cvec), self.NC
        s.idxA, s.idxB, s.sc = _ptr(self.idxA), _ptr(self.idxB if self.has_pb else None), _ptr(self.sc if self.NC else None)
        s.maskbits, s.actions = _ptr(self.maskbits), _ptr(self.actions)
        s.B, s.R, s.S, s.T, s.M, s.tstart, s.nchunk = self.B, self.R, self.S, self.T, self.M, self.tstart, self.nchunk
        s.clip, s.temp = self.clip, self.temp
        s.logp, s.lse = _ptr(self.logp), _ptr(self.lse)
        s.entropy = _ptr(self.entropy)
        if self.heads is not None:
            s.heads, s.heads_T = _ptr(self.heads), self.heads.shape[1]
        if self.dyn is not None:
            s.rem, s.dyn = _ptr(self.rem), _ptr(self.dyn)
        if self.nkc > 1:
            if self.scratch is None:
                n = int(_lib.load().eamrl_reeval_scratch_floats(self.R, self.T, self.M))
                self.scratch = torch.empty(n, dtype=torch.float32, device=self.buf.device)
            s.nkc, s.scratch = self.nkc, _ptr(self.scratch)
        return s

    def forward(self):
        if self.lse is None and not self.want_entropy:
            # a new tensor object: autograd makes the Function's output point at its node, and the node holds this plan --
            # returning self.logp itself would close a reference cycle that only the cyclic collector frees
            return self.logp.view_as(self.logp)
        lib = _lib.load()
        if self.want_entropy:
            self.entropy = torch.empty(self.R, self.T, dtype=torch.float32, device=self.buf.device)
            if self.lse is None:        # (the rollout's log-probs stay untouched: the kernel writes into a scratch)
                self.logp = torch.empty(self.R, self.T, dtype=torch.float32, device=self.buf.device)
                # the normaliser of this pass, for a backward that is handed an entropy gradient (it reads lse and entropy as
                # written here); a backward without one keeps recovering it from logp, as before
                self.lse_ent = torch.empty(self.R, self.T, dtype=torch.float32, device=self.buf.device)
        s = self._struct()
        if self.lse is None and self.want_entropy:
            s.lse = _ptr(self.lse_ent)
        _lib.check(lib.eamrl_reeval_forward(C.byref(s), _stream(self.buf)), "eamrl_reeval_forward")
        return self.logp.view_as(self.logp)         # (a new tensor object, see above)

    def backward(self, glogp, gent=None):
        """-> (dbuf [B, M, P*E], dgctx or None, dcvec or None).  gent [R, T] (optional): dL/d(entropy) per step, on a plan built
        with want_entropy=True whose forward() has run (eamrl_reeval.gent: single-chunk graphs; the library refuses the rest)."""
        if self.planes:
            raise ValueError("reeval backward: operands side by side [B, M, P * E] (a plane-layout decoder cache serves the forward only)")
        lib = _lib.load()
        glogp = glogp.contiguous()
        _chk(glogp, "grad of logp", torch.float32, (self.R, self.T))
        if gent is not None:
            if not self.want_entropy or self.entropy is None:
                raise ValueError("reeval backward: an entropy gradient needs a plan built with want_entropy=True whose forward() has run")
            gent = gent.contiguous()
            _chk(gent, "grad of entropy", torch.float32, (self.R, self.T))
        dev = self.buf.device
        dbuf = torch.zeros_like(self.buf)
        # (key chunks: per-chunk partials of dheads, then the per-chunk query gradients)
        dheads = torch.empty((2 * self.nkc if self.nkc > 1 else 1) * self.R, self.T, self.E, dtype=torch.float32, device=dev)
        dg = torch.zeros_like(self.gctx) if self.gctx is not None else None
        dc = torch.zeros_like(self.cvec) if self.NC else None
        s = self._struct()
        E4 = self.E * 4
        base = dbuf.data_ptr()
        s.glogp, s.dheads = _ptr(glogp), _ptr(dheads)
        s.dK, s.dV, s.dLp, s.dPa = (C.c_void_p(base + i * E4) for i in range(4))
        s.dPb = C.c_void_p(base + 4 * E4) if self.has_pb else None
        s.ldg = dbuf.shape[2]
        s.dgctx, s.dCvec = _ptr(dg), _ptr(dc)
        self.ddyn = torch.zeros_like(self.dyn) if self.dyn is not None else None      # read by the caller (SDVRP)
        s.ddyn = _ptr(self.ddyn)
        if gent is not None:
            s.gent = _ptr(gent)
            if self.lse is None:
                s.lse = _ptr(self.lse_ent)
        _lib.check(lib.eamrl_reeval_backward(C.byref(s), _stream(self.buf)), "eamrl_reeval_backward")
        return dbuf, dg, dc

    def backward_lp(self, glogp, out=None):
        """-> dLp [B, M, E] = d(sum glogp * logp)/dLp and nothing else (eamrl_reeval_backward_lp): the gradient of an adapted logit
        key (EAS-Emb).  `out` is accumulated into (+=).  Single-chunk graphs without a dynamic embedding (the library refuses any
        other plan before it launches anything); works on a plan that reads a decoder cache in place (slots=)."""
        lib = _lib.load()
        glogp = glogp.contiguous()
        _chk(glogp, "grad of logp", torch.float32, (self.R, self.T))
        if out is None:
            out = torch.zeros(self.B, self.M, self.E, dtype=torch.float32, device=self.buf.device)
        _chk(out, "dLp", torch.float32, (self.B, self.M, self.E))
        s = self._struct()
        s.glogp, s.dLp, s.ldg = _ptr(glogp), _ptr(out), self.E
        _lib.check(lib.eamrl_reeval_backward_lp(C.byref(s), _stream(self.buf)), "eamrl_reeval_backward_lp")
        return out

    def backward_layer(self, glogp, layer, out=None):
        """-> {"W1", "b1", "W2", "b2"}: d(sum glogp * logp)/d(layer parameters) of an EAS-Lay layer (eamrl_eas_layer_backward), in
        the parameters' own layout ([B, E * E] fragment order, [B, E]).  layer: the dict of `eas_layer_operands`; the plan's
        log-probs (or lse) and rollout heads must come from a rollout WITH that layer.  `out` (the same dict shape) is
        accumulated into (+=).  The library refuses plans above 112 nodes, with a dynamic embedding or without rollout heads
        before it launches anything."""
        lib = _lib.load()
        glogp = glogp.contiguous()
        _chk(glogp, "grad of logp", torch.float32, (self.R, self.T))
        ls = _eas_layer_struct(layer, self.B, self.E)
        if out is None:
            out = {n: torch.zeros(self.B, self.E * (self.E if n[0] == "W" else 1), dtype=torch.float32, device=self.buf.device)
                   for n in ("W1", "b1", "W2", "b2")}
        for n in ("W1", "b1", "W2", "b2"):
            _chk(out[n], f"d{n}", torch.float32, (self.B, self.E * (self.E if n[0] == "W" else 1)))
        ls.dW1, ls.db1, ls.dW2, ls.db2 = (out[n].data_ptr() for n in ("W1", "b1", "W2", "b2"))
        s = self._struct()
        s.glogp = _ptr(glogp)
        _lib.check(lib.eamrl_eas_layer_backward(C.byref(s), C.byref(ls), _stream(self.buf)), "eamrl_eas_layer_backward")
        return out


# ------------------------------------------------------------------------------------------------------
# environment transitions
# ------------------------------------------------------------------------------------------------------
def tsp_step_(mask, first, cur, istep, action, done):
    lib = _lib.load()
    R, N = mask.shape
    _chk(mask, "action_mask", torch.bool, (R, N))
    for nm, t in (("first_node", first), ("current_node", cur), ("i", istep), ("action", action)):
        _chk(t, nm, torch.int64)
        if t.numel() != R:
            raise ValueError(f"{nm} must have {R} elements")
    _chk(done, "done", torch.bool)
    if done.numel() != R:
        raise ValueError("done must have R elements")
    _lib.check(lib.eamrl_tsp_step(_ptr(_bytes(mask)), _ptr(first), _ptr(cur), _ptr(istep), _ptr(action),
                                  _ptr(_bytes(done)), R, N, _stream(mask)), "eamrl_tsp_step")


def cvrp_mask_(visited, used, vcap, demand, cur, mask):
    lib = _lib.load()
    R, M = visited.shape
    B, N = demand.shape
    if M != N + 1 or R % B:
        raise ValueError("cvrp_mask: shape mismatch")
    _chk(visited, "visited", torch.uint8)
    _chk(mask, "action_mask", torch.bool, (R, M))
    for nm, t in (("used_capacity", used), ("vehicle_capacity", vcap)):
        _chk(t, nm, torch.float32)
        if t.numel() != R:
            raise ValueError(f"{nm} must have {R} elements")
    _chk(demand, "demand", torch.float32)
    _chk(cur, "current_node", torch.int64)
    _lib.check(lib.eamrl_cvrp_mask(_ptr(visited), _ptr(used), _ptr(vcap), _ptr(demand), _ptr(cur), _ptr(_bytes(mask)),
                                   R, B, N, _stream(mask)), "eamrl_cvrp_mask")


def cvrp_step_mask_(visited, used, vcap, demand, cur, action, mask, done):
    lib = _lib.load()
    R, M = visited.shape
    B, N = demand.shape
    if M != N + 1 or R % B:
        raise ValueError("cvrp_step: shape mismatch")
    _chk(visited, "visited", torch.uint8)
    _chk(mask, "action_mask", torch.bool, (R, M))
    for nm, t in (("used_capacity", used), ("vehicle_capacity", vcap)):
        _chk(t, nm, torch.float32)
        if t.numel() != R:
            raise ValueError(f"{nm} must have {R} elements")
    _chk(demand, "demand", torch.float32)
    for nm, t in (("current_node", cur), ("action", action)):
        _chk(t, nm, torch.int64)
        if t.numel() != R:
            raise ValueError(f"{nm} must have {R} elements")
    _chk(done, "done", torch.bool)
    _lib.check(lib.eamrl_cvrp_step_mask(_ptr(visited), _ptr(used), _ptr(vcap), _ptr(demand), _ptr(cur), _ptr(action),
                                        _ptr(_bytes(mask)), _ptr(_bytes(done)), R, B, N, _stream(mask)),
               "eamrl_cvrp_step_mask")


# ------------------------------------------------------------------------------------------------------
# reward
# ------------------------------------------------------------------------------------------------------
def sdvrp_step_mask_(rem, used, vcap, cur, action, mask, done=None):
    """SDVRPEnv._step + get_action_mask in place (sdvrp/env.py:58-92,137-146); action None: mask only."""
    lib = _lib.load()
    R, M = rem.shape
    _chk(rem, "demand_with_depot", torch.float32)
    _chk(used, "used_capacity", torch.float32, (R,))
    _chk(vcap, "vehicle_capacity", torch.float32, (R,))
    _chk(cur, "current_node", torch.int64, (R,))
    _chk(mask, "action_mask", torch.bool, (R, M))
    if action is not None:
        _chk(action, "action", torch.int64, (R,))
        _chk(done, "done", torch.bool, (R,))
    _lib.check(lib.eamrl_sdvrp_step_mask(_ptr(rem), _ptr(used), _ptr(vcap), _ptr(cur), _ptr(action), _ptr(_bytes(mask)),
                                         _ptr(_bytes(done)), R, M, _stream(mask)),
               "eamrl_sdvrp_step_mask")
    return mask


def pctsp_step_mask_(visited, prize_tot, pen_tot, prize, penalty, cur, istep, action, mask, done=None):
    """PCTSPEnv._step + get_action_mask in place (pctsp/env.py:64-97,156-163); action None: mask only."""
    lib = _lib.load()
    R, M = visited.shape
    B = R if prize is None else prize.shape[0]
    if visited.dtype not in (torch.bool, torch.uint8):
        raise TypeError("visited must be bool or uint8")
    _chk(_bytes(visited), "visited", torch.uint8, (R, M))
    _chk(prize_tot, "cur_total_prize", torch.float32, (R,))
    _chk(mask, "action_mask", torch.bool, (R, M))
    if action is not None:
        _chk(prize, "real_prize", torch.float32, (B, M))
        _chk(cur, "current_node", torch.int64, (R,))
        _chk(istep, "i", torch.int64, (R,))
        _chk(action, "action", torch.int64, (R,))
        _chk(done, "done", torch.bool, (R,))
        if pen_tot is not None:
            _chk(pen_tot, "cur_total_penalty", torch.float32, (R,))
            _chk(penalty, "penalty", torch.float32, (B, M))
    _lib.check(lib.eamrl_pctsp_step_mask(_ptr(_bytes(visited)), _ptr(prize_tot), _ptr(pen_tot), _ptr(prize), _ptr(penalty),
                                         _ptr(cur), _ptr(istep), _ptr(action), _ptr(_bytes(mask)),
                                         _ptr(_bytes(done)), R, B, M, _stream(mask)),
               "eamrl_pctsp_step_mask")
    return mask


def pdp_step_mask_(visited, to_deliver, cur, action, mask, done=None):
    """PDPEnv._step and its mask in place (pdp/env.py:66-106); action None: mask only.  visited = ~available."""
    lib = _lib.load()
    R, M = visited.shape
    if M < 3 or M % 2 == 0:
        raise ValueError("pdp_step: the number of nodes (depot included) must be odd")
    for t, nm in ((visited, "visited"), (to_deliver, "to_deliver")):
        if t.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"{nm} must be bool or uint8")
        _chk(_bytes(t), nm, torch.uint8, (R, M))
    _chk(mask, "action_mask", torch.bool, (R, M))
    if action is not None:
        _chk(cur, "current_node", torch.int64, (R,))
        _chk(action, "action", torch.int64, (R,))
        _chk(done, "done", torch.bool, (R,))
    _lib.check(lib.eamrl_pdp_step_mask(_ptr(_bytes(visited)), _ptr(_bytes(to_deliver)), _ptr(cur), _ptr(action),
                                       _ptr(_bytes(mask)), _ptr(_bytes(done)), R, M,
                                       _stream(mask)), "eamrl_pdp_step_mask")
    return mask


def pdp_init_embedding(locs, Wd, bd, Wp, bp, Wl, bl, out=None):
    """PDPInitEmbedding.forward in one launch (init.py:347-372): [B, M, E] from locs [B, M, 2]; equals the three `linear`
    calls on the depot, pickup (x_p, y_p, x_d, y_d) and delivery features bit for bit."""
    lib = _lib.load()
    _chk(locs, "locs", torch.float32)
    B, M, two = locs.shape
    E = Wd.shape[0]
    if two != 2 or M < 3 or M % 2 == 0:
        raise ValueError("pdp_init_embedding: locs must be [B, N + 1, 2] with N even")
    _chk(Wd, "init_embed_depot.weight", torch.float32, (E, 2))
    _chk(Wp, "init_embed_pick.weight", torch.float32, (E, 4))
    _chk(Wl, "init_embed_delivery.weight", torch.float32, (E, 2))
    for b, nm in ((bd, "init_embed_depot.bias"), (bp, "init_embed_pick.bias"), (bl, "init_embed_delivery.bias")):
        if b is not None:
            _chk(b, nm, torch.float32, (E,))
    if out is None:
        out = torch.empty(B, M, E, device=locs.device, dtype=torch.float32)
    _chk(out, "out", torch.float32, (B, M, E))
    _lib.check(lib.eamrl_pdp_init_embedding(_ptr(locs), _ptr(Wd), _ptr(bd), _ptr(Wp), _ptr(bp), _ptr(Wl), _ptr(bl), _ptr(out),
                                            B, M, E, _stream(locs)), "eamrl_pdp_init_embedding")
    return out


def cvrptw_step_mask_(visited, used, vcap, demand, cur, time, locs, tw, dur, action, mask, done=None):
    """CVRPTWEnv._step + get_action_mask in place (cvrptw/env.py:103-138); action None: mask only.
    tw [B, M, 2] and dur [B, M] as float32."""
    lib = _lib.load()
    R, M = visited.shape
    B, N = demand.shape
    if N + 1 != M or R % B:
        raise ValueError("cvrptw_step: shape mismatch")
    _chk(visited, "visited", torch.uint8)
    _chk(used, "used_capacity", torch.float32, (R,))
    _chk(vcap, "vehicle_capacity", torch.float32, (R,))
    _chk(demand, "demand", torch.float32)
    _chk(cur, "current_node", torch.int64, (R,))
    _chk(time, "current_time", torch.float32, (R,))
    _chk(locs, "locs", torch.float32, (B, M, 2))
    _chk(tw, "time_windows", torch.float32, (B, M, 2))
    _chk(mask, "action_mask", torch.bool, (R, M))
    if action is not None:
        _chk(dur, "durations", torch.float32, (B, M))
        _chk(action, "action", torch.int64, (R,))
        _chk(done, "done", torch.bool, (R,))
    _lib.check(lib.eamrl_cvrptw_step_mask(_ptr(visited), _ptr(used), _ptr(vcap), _ptr(demand), _ptr(cur), _ptr(time),
                                          _ptr(locs), _ptr(tw), _ptr(dur), _ptr(action), _ptr(_bytes(mask)),
                                          _ptr(_bytes(done)), R, B, N, _stream(mask)),
               "eamrl_cvrptw_step_mask")
    return mask


def cvrptw_check_time(actions, locs, tw, dur):
    """-> device int32[2]: [0] = rows that start a service after its window closed (cvrptw/env.py:203-227)."""
    lib = _lib.load()
    _chk(actions, "actions", torch.int64)
    _chk(locs, "locs", torch.float32)
    B, M, _ = locs.shape
    _chk(tw, "time_windows", torch.float32, (B, M, 2))
    _chk(dur, "durations", torch.float32, (B, M))
    R, T = actions.shape
    bad = torch.zeros(2, device=actions.device, dtype=torch.int32)
    _lib.check(lib.eamrl_cvrptw_check_time(_ptr(actions), _ptr(locs), _ptr(tw), _ptr(dur), R, B, M, T, _ptr(bad),
                                           _stream(actions)), "eamrl_cvrptw_check_time")
    return bad


def op_step_mask_(visited, tour_len, prize_tot, prize, locs, maxlen, cur, istep, action, mask, done=None):
    """OPEnv._step + get_action_mask in place (op/env.py:69-102,149-165); action None: mask only."""
    lib = _lib.load()
    R, M = visited.shape
    _chk(locs, "locs", torch.float32)
    B = locs.shape[0]
    if tuple(locs.shape) != (B, M, 2) or R % B:
        raise ValueError("op_step: locs must be [B, M, 2] with R a multiple of B")
    _chk(_bytes(visited), "visited", torch.uint8, (R, M))
    _chk(tour_len, "tour_length", torch.float32, (R,))
    _chk(maxlen, "max_length", torch.float32, (B, M))
    _chk(cur, "current_node", torch.int64, (R,))
    _chk(mask, "action_mask", torch.bool, (R, M))
    if action is not None:
        _chk(istep, "i", torch.int64, (R,))
        _chk(action, "action", torch.int64, (R,))
        _chk(done, "done", torch.bool, (R,))
        if prize_tot is not None:
            _chk(prize_tot, "current_total_prize", torch.float32, (R,))
            _chk(prize, "prize", torch.float32, (B, M))
    _lib.check(lib.eamrl_op_step_mask(_ptr(_bytes(visited)), _ptr(tour_len), _ptr(prize_tot), _ptr(prize), _ptr(locs),
                                      _ptr(maxlen), _ptr(cur), _ptr(istep), _ptr(action), _ptr(_bytes(mask)),
                                      _ptr(_bytes(done)), R, B, M, _stream(mask)),
               "eamrl_op_step_mask")
    return mask


def op_reward(prize, actions):
    """OPEnv._get_reward (op/env.py:167-177): the collected prize."""
    lib = _lib.load()
    _chk(prize, "prize", torch.float32)
    B, M = prize.shape
    _chk(actions, "actions", torch.int64)
    R, T = actions.shape
    if R % B:
        raise ValueError("actions rows must be a multiple of the number of instances")
    out = torch.empty(R, dtype=torch.float32, device=prize.device)
    _lib.check(lib.eamrl_op_reward(_ptr(prize), _ptr(actions), _ptr(out), R, B, M, T, _stream(prize)), "eamrl_op_reward")
    return out


def op_check_solution(actions, locs, maxlen):
    """-> device int32[2]: (rows with a customer visited twice, rows longer than allowed)  (op/env.py:179-212)."""
    lib = _lib.load()
    _chk(actions, "actions", torch.int64)
    _chk(locs, "locs", torch.float32)
    B, M, _ = locs.shape
    _chk(maxlen, "max_length", torch.float32, (B, M))
    R, T = actions.shape
    bad = torch.zeros(2, device=actions.device, dtype=torch.int32)
    _lib.check(lib.eamrl_op_check_solution(_ptr(actions), _ptr(locs), _ptr(maxlen), R, B, M, T, _ptr(bad),
                                           _stream(actions)), "eamrl_op_check_solution")
    return bad


def pctsp_reward(locs, penalty, actions):
    """PCTSPEnv._get_reward (pctsp/env.py:165-187): saved penalties - (tour length + all penalties)."""
    lib = _lib.load()
    _chk(locs, "locs", torch.float32)
    B, M, _ = locs.shape
    _chk(penalty, "penalty", torch.float32, (B, M))
    _chk(actions, "actions", torch.int64)
    R, T = actions.shape
    if R % B:
        raise ValueError("actions rows must be a multiple of the number of instances")
    out = torch.empty(R, dtype=torch.float32, device=locs.device)
    _lib.check(lib.eamrl_pctsp_reward(_ptr(locs), _ptr(penalty), _ptr(actions), _ptr(out), R, B, M, T, _stream(locs)),
               "eamrl_pctsp_reward")
    return out


def tour_length_reward(locs, actions, with_depot):
    lib = _lib.load()
    _chk(locs, "locs", torch.float32)
    _chk(actions, "actions", torch.int64)
    B, M, two = locs.shape
    R, T = actions.shape
    if two != 2 or R % B:
        raise ValueError("tour_length: shape mismatch")
    out = torch.empty(R, device=locs.device, dtype=torch.float32)
    _lib.check(lib.eamrl_tour_length(_ptr(locs), _ptr(actions), _ptr(out), R, B, M, T, int(with_depot), _stream(locs)),
               "eamrl_tour_length")
    return out


def sum_logp(logp):
    lib = _lib.load()
    _need_gpu(logp, "logp")
    if logp.dtype != torch.float32 or logp.dim() != 2 or logp.stride(1) != 1:
        raise ValueError("sum_logp: [R, T] fp32 with unit inner stride required")
    R, T = logp.shape
    out = torch.empty(R, device=logp.device, dtype=torch.float32)
    _lib.check(lib.eamrl_sum_logp(_ptr(logp), logp.stride(0), _ptr(out), R, T, _stream(logp)), "eamrl_sum_logp")
    return out


MULTI_COPY_MAX = 16


def multi_copy_(pairs):
    """[(dst, src | None), ...] -> dst.copy_(src) / dst.zero_() for all of them in ONE launch per 16 segments
    (eamrl_multi_copy).  Tensors must be contiguous, on the same device, src of dst's dtype and size."""
    lib = _lib.load()
    segs = []
    for dst, src in pairs:
        _need_gpu(dst, "multi_copy dst")
        if not dst.is_contiguous():
            raise ValueError("multi_copy: dst must be contiguous")
        if src is not None:
            if src.dtype != dst.dtype or src.numel() != dst.numel() or not src.is_contiguous() or src.device != dst.device:
                raise ValueError("multi_copy: src must be a contiguous tensor of dst's dtype, size and device")
        if dst.numel():
            segs.append((dst, src))
    for i in range(0, len(segs), MULTI_COPY_MAX):
        part = segs[i:i + MULTI_COPY_MAX]
        n = len(part)
        srcs = (C.c_void_p * n)(*[None if s_ is None else s_.data_ptr() for _, s_ in part])
        dsts = (C.c_void_p * n)(*[d.data_ptr() for d, _ in part])
        nbytes = (C.c_int64 * n)(*[d.numel() * d.element_size() for d, _ in part])
        _lib.check(lib.eamrl_multi_copy(n, srcs, dsts, nbytes, _stream(part[0][0])), "eamrl_multi_copy")


def call_spec(entry, td, actions, vcap=None):
    """A `reward` / `check` entry (ops function, arguments) of an env_spec record on the tours `actions` [R, T]."""
    special = {env_spec.ACTION: actions, env_spec.NUM_LOC: td["locs"].shape[-2] - 1, env_spec.VCAP: vcap}
    return globals()[entry[0]](*(a if not isinstance(a, str) else special[a] if a in special else a[1:] if a[0] == "="
                                 else td[a].contiguous() for a in entry[1]))


def _row_capacity(vcap, R):
    """vehicle_capacity as one fp32 per row: [R], the per-instance values repeated for the rows of every start."""
    vc = vcap.reshape(-1).contiguous()
    if vc.numel() != R:
        vc = vc.repeat(R // vc.numel())
    return _chk(vc, "vehicle_capacity", torch.float32, (R,))


def rollout_finish(env_name, locs, actions, logp=None, demand=None, vcap=None, want_reward=True, bad=None):
    """Reward, summed log-likelihood and validity counters of TSP / CVRP tours in one launch (eamrl_rollout_finish):
    bit-identical to tour_length_reward / sum_logp / check_solution.  bad: int32[2] device tensor to add to, or None.
    -> (reward [R] | None, ll [R] | None)."""
    lib = _lib.load()
    _chk(locs, "locs", torch.float32)
    _chk(actions, "actions", torch.int64)
    B, M, _ = locs.shape
    R, T = actions.shape
    if R % B:
        raise ValueError("rollout_finish: rows must be a multiple of the number of instances")
    reward = torch.empty(R, device=locs.device, dtype=torch.float32) if want_reward else None
    ll, ld = None, 0
    if logp is not None:
        _need_gpu(logp, "logp")
        if logp.dtype != torch.float32 or logp.shape != actions.shape or logp.stride(1) != 1:
            raise ValueError("rollout_finish: logp must be [R, T] fp32 with unit inner stride")
        ll, ld = torch.empty(R, device=locs.device, dtype=torch.float32), logp.stride(0)
    vc = None
    if env_name == "cvrp" and bad is not None:
        _chk(demand, "demand", torch.float32, (B, M - 1))
        vc = _row_capacity(vcap, R)
    _lib.check(lib.eamrl_rollout_finish(ENVS[env_name], _ptr(locs), _ptr(actions), _ptr(logp), ld, _ptr(demand), _ptr(vc),
                                        _ptr(reward), _ptr(ll), _ptr(bad), R, B, M, T, _stream(locs)), "eamrl_rollout_finish")
    return reward, ll


def check_solution(env_name, actions, demand=None, vcap=None, num_loc=None):
    """-> device int32[2]: (invalid tours, over-capacity rows); sdvrp: (rows with demand left, double depot visits)."""
    lib = _lib.load()
    _chk(actions, "actions", torch.int64)
    R, T = actions.shape
    bad = torch.zeros(2, device=actions.device, dtype=torch.int32)
    if env_name == "tsp":
        N, B = (T if num_loc is None else num_loc), R
        _lib.check(lib.eamrl_check_solution(ENV_TSP, _ptr(actions), None, None, R, B, N, T, _ptr(bad), _stream(actions)),
                   "eamrl_check_solution")
    elif env_name == "pdp":         # (not a permutation of 1..N, delivery before pickup); num_loc = N, T = N or N + 1
        N = (T if num_loc is None else int(num_loc))
        _lib.check(lib.eamrl_check_solution(ENV_PDP, _ptr(actions), None, None, R, R, N, T, _ptr(bad), _stream(actions)),
                   "eamrl_check_solution")
    elif env_name == "pctsp":       # demand = real_prize [B, N+1]
        _chk(demand, "real_prize", torch.float32)
        B, M = demand.shape
        _lib.check(lib.eamrl_check_solution(ENV_PCTSP, _ptr(actions), _ptr(demand), None, R, B, M - 1, T, _ptr(bad),
                                            _stream(actions)), "eamrl_check_solution")
    else:
        _chk(demand, "demand", torch.float32)
        B, N = demand.shape
        vc = _row_capacity(vcap, R)
        _lib.check(lib.eamrl_check_solution(ENVS[env_name], _ptr(actions), _ptr(demand), _ptr(vc), R, B, N, T, _ptr(bad),
                                            _stream(actions)), "eamrl_check_solution")
    return bad


# the sizes at which eamrl_tsp_two_opt switches variant (include/eamrl.h EAMRL_TWO_OPT_*): results do not depend on them
TWO_OPT_WAVE_MAX, TWO_OPT_BLOCK256_MAX, TWO_OPT_LDS_MATRIX_MAX = 48, 256, 120


def tsp_two_opt(actions, locs=None, distances=None, max_iterations=1000):
    """Best-improvement 2-opt on TSP tours, every sweep of every tour in one launch (eamrl_tsp_two_opt;
    rl4co/envs/routing/tsp/local_search.py:17-79).  actions [B, N] int64 (not modified); exactly one of locs [B, N, 2]
    and distances [B, N, N] (fp32).  -> (tours [B, N] int64, iters [B] int32 = sweeps run, status int32[1] = number of
    rows that are not permutations of 0..N-1; those are returned unchanged).  Enqueued on the current stream, no host
    sync: read `status` when convenient."""
    lib = _lib.load()
    _chk(actions, "actions", torch.int64)
    if actions.dim() != 2:
        raise ValueError(f"actions must be [B, N], got {tuple(actions.shape)}")
    B, N = actions.shape
    if (locs is None) == (distances is None):
        raise ValueError("tsp_two_opt: pass exactly one of locs and distances")
    if locs is not None:
        _chk(locs, "locs", torch.float32, (B, N, 2))
    else:
        _chk(distances, "distances", torch.float32, (B, N, N))
    if not 2 <= N <= 1024:
        raise ValueError(f"tsp_two_opt: 2 <= N <= 1024 required, got {N}")
    max_iterations = int(max_iterations)
    if max_iterations < 0:
        raise ValueError("tsp_two_opt: max_iterations must be >= 0")
    dev = actions.device
    tours = torch.empty_like(actions)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.eamrl_tsp_two_opt(_ptr(locs), _ptr(distances), _ptr(actions), _ptr(tours), _ptr(iters), _ptr(status), B, N,
                                     max_iterations, _stream(actions)), "eamrl_tsp_two_opt")
    return tours, iters, status


# ------------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------------
def beam_topk(logprobs, parent, B: int, beam_width: int):
    """Per instance the beam_width best (beam, node) candidates of a beam-search step.
    -> node [R] i64, beam [R] i32, cum [R] f32, step_logp [R] f32 with R = beam_width * B (rows "(w b)")."""
    lib = _lib.load()
    R, M = logprobs.shape
    if R != beam_width * B:
        raise ValueError("beam_topk: rows must be beam_width * B")
    _chk(logprobs, "logprobs", torch.float32)
    _chk(parent, "parent", torch.float32, (R,))
    dev = logprobs.device
    node = torch.empty(R, dtype=torch.int64, device=dev)
    beam = torch.empty(R, dtype=torch.int32, device=dev)
    cum = torch.empty(R, dtype=torch.float32, device=dev)
    slp = torch.empty(R, dtype=torch.float32, device=dev)
    _lib.check(lib.eamrl_beam_topk(_ptr(logprobs), _ptr(parent), B, beam_width, M, _ptr(node), _ptr(beam), _ptr(cum),
                                   _ptr(slp), _stream(logprobs)), "eamrl_beam_topk")
    return node, beam, cum, slp


def ea_num_pairs(selection_rate: float, pop_size: int) -> int:
    """Crossover pairs per generation of EA.run (elites // 2; int(rate*S) elites, 0 -> all, S <= 2 -> all)."""
    if pop_size <= 2:
        ne = pop_size
    else:
        ne = int(selection_rate * pop_size)
        ne = pop_size if ne <= 0 else min(ne, pop_size)
    return ne // 2


EA_KERNELS = ("lds", "large")          # EAMRL_EA_KERNEL_* of include/eamrl.h


def ea_kernel(env_name: str, S: int, N: int, L: int = 0, kernel: str | None = None) -> str:
    """The kernel an EA.run of population size S on N nodes / customers with rows of L entries runs on: "lds" (one
    workgroup per instance, populations in LDS: up to 128 x 128) or "large" (one launch per phase, populations in device
    memory: TSP and CVRP up to 1024) -- the library's own dispatch (eamrl_ea_kernel).  kernel="lds" / "large" asks for that
    path instead.  ValueError with the limit where no kernel, or not the requested one, serves the shape."""
    if kernel not in (None,) + EA_KERNELS:
        raise ValueError(f"ea kernel must be None, 'lds' or 'large', not {kernel!r}")
    lib = _lib.load()
    rc = lib.eamrl_ea_kernel(ENVS[env_name], int(S), int(N), int(L))
    if rc < 0:
        raise ValueError(f"EA.run on {env_name} with population {S}, {N} nodes, rows of {L or N}: "
                         f"{lib.eamrl_last_error().decode()}")
    served = EA_KERNELS[rc]
    if kernel == "lds" and served != "lds":
        raise ValueError(f"EA.run on {env_name} with population {S}, {N} nodes, rows of {L or N} is beyond the LDS kernel "
                         "(TSP: S, N <= 128; CVRP: S <= 128, N <= 127, L <= 256, S * L <= 24000)")
    if kernel == "large" and env_name not in ("tsp", "cvrp"):
        raise ValueError(f"the large EA path is built for tsp and cvrp, not {env_name} (S <= 128, N <= 127, L <= 128 there)")
    return kernel or served


def _ea_scratch(lib, env_name, B, S, L, selection_rate, device):
    nbytes = lib.eamrl_ea_large_scratch_bytes(ENVS[env_name], B, S, L, float(selection_rate))
    if nbytes == 0:
        raise ValueError(lib.eamrl_last_error().decode())
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def ea_tsp_run_(locs, pop, num_generations, mutation_rate, crossover_rate, selection_rate, cross_rand, cross_idx,
                mut_rand, mut_idx, kernel=None):
    """In place on pop [B, S, N] (int64); returns fitness [B, S].  Draw tensors: see include/eamrl.h.  kernel: see
    ea_kernel."""
    lib = _lib.load()
    B, S, N = pop.shape
    kernel = ea_kernel("tsp", S, N, N, kernel)        # the shape's limits first: a ValueError needs no device
    _chk(locs, "locs", torch.float32)
    _chk(pop, "pop", torch.int64)
    if locs.shape != (B, N, 2):
        raise ValueError(f"ea_tsp_run: locs {tuple(locs.shape)} does not match pop {tuple(pop.shape)}")
    P = ea_num_pairs(selection_rate, S)
    G = int(num_generations)
    if G > 0 and P > 0:
        _chk(cross_rand, "cross_rand", torch.float64, (G, B, P))
        _chk(cross_idx, "cross_idx", torch.int32, (G, B, P, 2))
        _chk(mut_rand, "mut_rand", torch.float64, (G, B, 2 * P))
        _chk(mut_idx, "mut_idx", torch.int32, (G, B, 2 * P, 2))
    fitness = torch.empty(B, S, device=pop.device, dtype=torch.float32)
    nul = lambda t: _ptr(t) if (G > 0 and P > 0) else None
    args = (_ptr(locs), _ptr(pop), _ptr(fitness), B, S, N, G, float(mutation_rate), float(crossover_rate),
            float(selection_rate), nul(cross_rand), nul(cross_idx), nul(mut_rand), nul(mut_idx))
    if kernel == "large":
        scratch, nbytes = _ea_scratch(lib, "tsp", B, S, N, selection_rate, pop.device)
        _lib.check(lib.eamrl_ea_tsp_run_large(*args, _ptr(scratch), nbytes, _stream(pop)), "eamrl_ea_tsp_run_large")
    else:
        _lib.check(lib.eamrl_ea_tsp_run(*args, _stream(pop)), "eamrl_ea_tsp_run")
    return fitness


def ea_cvrp_run_(locs, demand, vcap, pop, num_generations, mutation_rate, crossover_rate, selection_rate, top_k,
                 init_mut_rand, init_mut_u, cross_rand, cross_u, mut_rand, mut_u, kernel=None):
    """In place on pop [B, S, L] (int64 action rows, 0 = depot); returns fitness [B, S].  See include/eamrl.h.  kernel: see
    ea_kernel."""
    lib = _lib.load()
    B, S, L = pop.shape
    N = demand.shape[-1]
    kernel = ea_kernel("cvrp", S, N, L, kernel)
    _chk(pop, "pop", torch.int64)
    _chk(locs, "locs", torch.float32, (B, N + 1, 2))
    _chk(demand, "demand", torch.float32, (B, N))
    _chk(vcap, "vcap", torch.float32, (B,))
    P = ea_num_pairs(selection_rate, S)
    G = int(num_generations)
    _chk(init_mut_rand, "init_mut_rand", torch.float64, (B, S))
    _chk(init_mut_u, "init_mut_u", torch.float64, (B, S, 3))
    if G > 0 and P > 0:
        _chk(cross_rand, "cross_rand", torch.float64, (G, B, P))
        _chk(cross_u, "cross_u", torch.float64, (G, B, P))
        _chk(mut_rand, "mut_rand", torch.float64, (G, B, 2 * P))
        _chk(mut_u, "mut_u", torch.float64, (G, B, 2 * P, 3))
    fitness = torch.empty(B, S, device=pop.device, dtype=torch.float32)
    nul = lambda t: _ptr(t) if (G > 0 and P > 0) else None
    args = (_ptr(locs), _ptr(demand), _ptr(vcap), _ptr(pop), _ptr(fitness), B, S, N, L, G, float(mutation_rate),
            float(crossover_rate), float(selection_rate), int(bool(top_k)), _ptr(init_mut_rand), _ptr(init_mut_u),
            nul(cross_rand), nul(cross_u), nul(mut_rand), nul(mut_u))
    if kernel == "large":
        scratch, nbytes = _ea_scratch(lib, "cvrp", B, S, L, selection_rate, pop.device)
        _lib.check(lib.eamrl_ea_cvrp_run_large(*args, _ptr(scratch), nbytes, _stream(pop)), "eamrl_ea_cvrp_run_large")
    else:
        _lib.check(lib.eamrl_ea_cvrp_run(*args, _stream(pop)), "eamrl_ea_cvrp_run")
    return fitness


def ea_prize_run_(env_name, locs, prize, aux, pop, num_generations, mutation_rate, crossover_rate, selection_rate, top_k,
                  init_mut_rand, init_mut_u, cross_rand, cross_u, mut_rand, mut_u):
    """PCTSP / OP EA.run, in place on pop [B, S, L] (int64 action rows, 0 = depot); returns fitness [B, S].
    prize / aux [B, N+1] with the depot first (aux: PCTSP penalty, OP max_length).  See include/eamrl.h."""
    lib = _lib.load()
    if env_name not in ("pctsp", "op"):
        raise ValueError("ea_prize_run: env must be pctsp or op")
    B, S, L = pop.shape
    M = locs.shape[1]
    ea_kernel(env_name, S, M - 1, L)
    _chk(pop, "pop", torch.int64)
    _chk(locs, "locs", torch.float32, (B, M, 2))
    _chk(prize, "prize", torch.float32, (B, M))
    _chk(aux, "penalty / max_length", torch.float32, (B, M))
    P = ea_num_pairs(selection_rate, S)
    G = int(num_generations)
    _chk(init_mut_rand, "init_mut_rand", torch.float64, (B, S))
    _chk(init_mut_u, "init_mut_u", torch.float64, (B, S, 2))
    if G > 0 and P > 0:
        _chk(cross_rand, "cross_rand", torch.float64, (G, B, P))
        if env_name == "op":
            _chk(cross_u, "cross_u", torch.float64, (G, B, P))
        _chk(mut_rand, "mut_rand", torch.float64, (G, B, 2 * P))
        _chk(mut_u, "mut_u", torch.float64, (G, B, 2 * P, 2))
    fitness = torch.empty(B, S, device=pop.device, dtype=torch.float32)
    nul = lambda t: _ptr(t) if (G > 0 and P > 0 and t is not None) else None
    _lib.check(lib.eamrl_ea_prize_run(ENVS[env_name], _ptr(locs), _ptr(prize), _ptr(aux), _ptr(pop), _ptr(fitness), B, S,
                                      M - 1, L, G, float(mutation_rate), float(crossover_rate), float(selection_rate),
                                      int(bool(top_k)), _ptr(init_mut_rand), _ptr(init_mut_u), nul(cross_rand),
                                      nul(cross_u), nul(mut_rand), nul(mut_u), _stream(pop)), "eamrl_ea_prize_run")
    return fitness


class DecodeCache:
    """Device-resident decoder cache (struct eamrl_cache).

    Two layouts of the same E-wide per-node rows (the kernels take base pointers and a row stride, so both work):
      * slot-major, one [B, M, ld] fp32 buffer with the rows of a node side by side -- graphs up to 128 nodes, where
        the register-resident kernel reads everything once:
            TSP : K | V | L | P_first | P_current | Lp        (ld = 6E)
            CVRP: K | V | L | P_current | Lp                  (ld = 5E)
      * plane-major, [P, B, M, E] (ld = E) -- larger graphs, where the streaming kernel re-reads one kind of row per
        stage and step: a stage then walks one dense plane instead of 512 bytes out of every 2.5-3 KB.
    K, V, L are AttentionModelDecoder's glimpse_key / glimpse_val / logit_key
    (zoo/am/decoder.py:206-235); P_* and Lp are the weight folds described in DESIGN.md.
    """

    def __init__(self, env_name, buf, cvec, gctx, embeddings, num_heads, dyn=None, embed_dim=None):
        self.env_name, self.buf, self.cvec, self.gctx = env_name, buf, cvec, gctx
        self.dyn = dyn          # sdvrp: [3, E] dynamic-embedding vectors (key, value, folded logit key)
        self.node_embeddings = embeddings      # None when the fused encoder kept them in LDS (nobody asked for them)
        self.E = embeddings.shape[-1] if embeddings is not None else int(embed_dim)
        self.H = num_heads
        self.slots = slot_map(env_name)
        self.planes = buf.dim() == 4
        if self.planes:
            P, self.B, self.M, self.ld = buf.shape
            assert P == len(self.slots) and self.ld == self.E
        else:
            self.B, self.M, self.ld = buf.shape
            assert self.ld == len(self.slots) * self.E

    def view(self, name):
        i = self.slots[name]
        return self.buf[i] if self.planes else self.buf[..., i * self.E:(i + 1) * self.E]

    # the reference's vocabulary (PrecomputedCache fields, zoo/am/decoder.py:22-41)
    @property
    def glimpse_key(self):
        return self.view("K")

    @property
    def glimpse_val(self):
        return self.view("V")

    @property
    def logit_key(self):
        return self.view("L")

    @property
    def graph_context(self):
        return self.gctx if self.gctx is not None else 0

    def slot_ptr(self, name):
        """Address of the rows `name` (node 0 of instance 0; row stride ld floats) in either layout."""
        return self.buf.data_ptr() + self.slots[name] * (self.B * self.M * self.E * 4 if self.planes else self.E * 4)

    def struct(self):
        c = _lib.Cache()
        c.K, c.V, c.Lp, c.Pa = (C.c_void_p(self.slot_ptr(n)) for n in ("K", "V", "Lp", "Pa"))
        c.Pb = C.c_void_p(self.slot_ptr("Pb")) if "Pb" in self.slots else None
        c.cvec, c.gctx = _ptr(self.cvec), _ptr(self.gctx)
        c.ld, c.B, c.M, c.E, c.H = self.ld, self.B, self.M, self.E, self.H
        c.dyn = _ptr(self.dyn)
        return c


def slot_map(env_name):
    names = ["K", "V", "L", "Pa", "Pb", "Lp"] if env_spec.ENV_SPECS[env_name].has_pb else ["K", "V", "L", "Pa", "Lp"]
    return {n: i for i, n in enumerate(names)}


class RolloutState:
    """Flat per-row state tensors (struct eamrl_state) for R = S*B rows.  Every slot of the struct is an attribute, None
    where the env does not use it; which slots an env uses, and what they mean there, is env_spec.ENV_SPECS[env].fields."""
    first = cur = istep = used = vcap = demand = mask = visited = done = rem = locs = time = tw = dur = None
    heads_out = to_deliver = None           # heads_out: [R, t_max, E] while `rollout` captures the glimpse outputs

    def __init__(self, env_name, R, M, device, demand=None):
        self.env_name, self.R, self.M = env_name, R, M
        self.done = torch.zeros(R, dtype=torch.bool, device=device)
        self.mask = torch.ones(R, M, dtype=torch.bool, device=device)
        # (the per-instance tensors are the caller's: `demand`; locs, tw, dur set afterwards)
        for f in filter(lambda f: f.per_row, env_spec.ENV_SPECS[env_name].fields):
            v = (torch.ones if f.reset == "ones" else torch.zeros)(
                (R,) + env_spec.dims(f.shape, M, device=True), device=device,
                dtype=torch.uint8 if f.dtype == torch.bool else f.dtype)        # (bool planes are passed as bytes anyway)
            if f.reset.startswith("depot"):
                v[:, :1 if f.reset == "depot" else (M - 1) // 2 + 1] = 1
            setattr(self, f.slot, v)
        self.demand = demand
        if self.to_deliver is not None:     # the reset state of PDPEnv: depot visited, depot and pickups to deliver, mask = their AND
            self.mask = (self.visited == 0) & (self.to_deliver != 0)

    def reorder_(self, idx):
        """Rows taken from rows `idx` (beam search: every beam continues the state of its parent beam).  vcap is
        per instance and the row order keeps r % B, so it needs no reordering, nor do the per-instance tensors.  Every
        per-row slot of the env must be set (as `__init__` and `policy.state_from_td` leave it)."""
        rows = [f.slot for f in env_spec.ENV_SPECS[self.env_name].fields if f.per_row and f.slot != "vcap"]
        for name in ["mask", "done"] + rows:
            setattr(self, name, getattr(self, name).index_select(0, idx).contiguous())

    def struct(self):
        s = _lib.State()
        for name, _ in s._fields_:
            t = getattr(self, name)
            if t is not None:               # (a bool tensor and its uint8 view share the address)
                setattr(s, name, t.data_ptr())
        return s


def _validate_state(st: RolloutState, cache: DecodeCache):
    R, M = st.R, st.M
    if M != cache.M or R % cache.B:
        raise ValueError("decode: state / cache shape mismatch")
    spec = env_spec.ENV_SPECS[st.env_name]
    _chk(st.mask, "action_mask", torch.bool, (R, M))
    _chk(st.done, "done", torch.bool, (R,))
    if st.to_deliver is not None and (M < 3 or M % 2 == 0):
        raise ValueError("decode: PDP needs an odd number of nodes (depot + pickups + deliveries)")
    for f in spec.fields:
        t, dtype = getattr(st, f.slot), f.dtype
        if dtype == torch.bool and isinstance(t, torch.Tensor):     # bool planes: bool or their uint8 storage
            t, dtype = _bytes(t), torch.uint8
        _chk(t, f.key, dtype, (R if f.per_row else cache.B,) + env_spec.dims(f.shape, M, device=True))
    if st.rem is not None:      # the remaining demands are what the dynamic embedding multiplies
        _chk(cache.dyn, "dynamic embedding vectors", torch.float32, (3, cache.E))
    if spec.n_state_cols > 1:
        _chk(cache.cvec, "context state columns", torch.float32, (spec.n_state_cols * cache.E,))


def decode_step(st: RolloutState, cache: DecodeCache, mode="greedy", noise=None, given=None, clip=10.0, temp=1.0,
                fuse_env_step=False, want_logprobs=False, want_logits=False, status=None, top_k=0, top_p=0.0):
    """One decode step for all rows.  -> (action [R], logp [R], logprobs [R,M] | None, logits [R,M] | None)."""
    lib = _lib.load()
    _validate_state(st, cache)
    R, M, dev = st.R, st.M, st.mask.device
    action = torch.empty(R, dtype=torch.int64, device=dev)
    logp = torch.empty(R, dtype=torch.float32, device=dev)
    lps = torch.empty(R, M, dtype=torch.float32, device=dev) if want_logprobs else None
    lgs = torch.empty(R, M, dtype=torch.float32, device=dev) if want_logits else None
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    if noise is not None:
        _chk(noise, "noise", torch.float32, (R, M))
    if given is not None:
        _chk(given, "given actions", torch.int64, (R,))
    cs, ss = cache.struct(), st.struct()
    _lib.check(lib.eamrl_am_decode_step(ENVS[st.env_name], C.byref(cs), C.byref(ss), R, MODES[mode], _ptr(noise),
                                        _ptr(given), float(clip), float(temp), int(top_k), float(top_p),
                                        int(fuse_env_step), _ptr(action),
                                        _ptr(logp), _ptr(lps), _ptr(lgs), _ptr(status), _stream(st.mask)),
               "eamrl_am_decode_step")
    return action, logp, lps, lgs, status


def _seed64(seed):
    """A Python int seed as the uint64 the library takes (the low 64 bits)."""
    return C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)


def exp1_noise(seed: int, R: int, T: int, M: int, device="cuda", seed_dev=None):
    """[R, T, M] Exp(1) draws of the library's counter-based generator (eamrl_exp1_noise): what a seeded rollout uses.
    seed_dev: optional int64 device tensor [1] XOR-ed into the seed on the device."""
    lib = _lib.load()
    out = torch.empty(R, T, M, dtype=torch.float32, device=device)
    _need_gpu(out, "noise")
    _lib.check(lib.eamrl_exp1_noise(_seed64(seed), _ptr(seed_dev), _ptr(out), R, T, M,
                                    _stream(out)), "eamrl_exp1_noise")
    return out


# EAMRL_PROBE_* / EAMRL_WPROBE_* of include/eamrl.h (test support: the functions of csrc/dmath.hpp one at a time)
MATH_PROBES = {"expf": 0, "expf2": 1, "expf2_nonpos": 2, "expf2_nonpos_x2": 3, "expf4": 4, "expf4_nonpos": 5, "logf": 6,
               "logf4": 7, "rcpf": 8, "tanhf": 9, "tanhf2": 10, "tanhf4": 11, "exp1_from_bits": 12, "philox": 13}
WAVE_PROBES = {"tree_sum": 0, "max": 1, "argmax": 2, "vmax": 3, "vmax3": 4, "vmax5": 5, "zrot": 6, "z_total_rel": 7}


def math_probe(fn: str, bits):
    """y[i] = f(x[i]) for one function of dmath.hpp (MATH_PROBES); `bits` is an int32 device tensor holding the float32 (or
    noise word) bit patterns, the result likewise.  Elements 4 g .. 4 g + 3 fill the slots of one wide call; the length must
    be a multiple of 4.  "philox": bits [G, 6] (counter, key) -> [G, 4] words."""
    lib = _lib.load()
    _need_gpu(bits, "bits")
    if bits.dtype != torch.int32 or not bits.is_contiguous():
        raise TypeError("math_probe: bits must be a contiguous int32 tensor (bit patterns)")
    if fn == "philox":
        if bits.dim() != 2 or bits.shape[1] != 6:
            raise ValueError("math_probe: philox takes [G, 6] words")
        out = torch.empty(bits.shape[0], 4, dtype=torch.int32, device=bits.device)
    else:
        out = torch.empty_like(bits)
    rc = lib.eamrl_math_probe(MATH_PROBES[fn], _ptr(bits), _ptr(out), out.numel(), _stream(bits))
    if rc != 0:
        raise RuntimeError(f"eamrl_math_probe({fn}) failed ({rc}): n = {out.numel()} must be a multiple of 4")
    return out


def wave_probe(fn: str, v_bits, idx=None):
    """One wavefront primitive of dmath.hpp (WAVE_PROBES) on [W, 64] cases, one 64-lane wavefront each; v_bits int32 bit
    patterns, idx int32 [W, 64] (argmax: the lane's index; zrot / z_total_rel: idx[w, 0] = start, idx[w, 1] = n1).
    -> out_v [W, 64] int32 bit patterns of what every lane ends with (argmax: (out_v, out_i))."""
    lib = _lib.load()
    _need_gpu(v_bits, "v_bits")
    if v_bits.dtype != torch.int32 or not v_bits.is_contiguous() or v_bits.dim() != 2 or v_bits.shape[1] != 64:
        raise TypeError("wave_probe: v_bits must be a contiguous int32 [W, 64] tensor")
    needs_idx = fn in ("argmax", "zrot", "z_total_rel")
    if needs_idx:
        if idx is None or idx.dtype != torch.int32 or not idx.is_contiguous() or idx.shape != v_bits.shape \
                or idx.device != v_bits.device:
            raise TypeError(f"wave_probe: {fn} needs an int32 idx of v_bits' shape on its device")
    out_v = torch.empty_like(v_bits)
    out_i = torch.empty_like(v_bits) if fn == "argmax" else None
    rc = lib.eamrl_wave_probe(WAVE_PROBES[fn], _ptr(v_bits), _ptr(idx if needs_idx else None), _ptr(out_v), _ptr(out_i),
                              v_bits.shape[0], _stream(v_bits))
    if rc != 0:
        raise RuntimeError(f"eamrl_wave_probe({fn}) failed ({rc})")
    return (out_v, out_i) if fn == "argmax" else out_v


ROLLOUT_KERNELS = ("ms_mfma", "resident", "stream")       # EAMRL_KERNEL_* of include/eamrl.h


def rollout_kernel(st_or_env_name, cache, R, t_max, top_k=0, top_p=0.0) -> str:
    """The kernel `rollout` runs for this shape: "ms_mfma" (start-sharing MFMA kernel), "resident" (register-resident) or
    "stream".  Host only: nothing is launched, and the answer comes from the function the dispatcher itself branches on
    (eamrl_rollout_kernel).  `cache` is a DecodeCache or a `_lib.Cache` struct (only its shape fields are read)."""
    env_name = st_or_env_name if isinstance(st_or_env_name, str) else st_or_env_name.env_name
    cs = cache if isinstance(cache, _lib.Cache) else cache.struct()
    rc = _lib.load().eamrl_rollout_kernel(ENVS[env_name], C.byref(cs), int(R), int(t_max), int(top_k), float(top_p))
    _lib.check(min(rc, 0), "eamrl_rollout_kernel")
    return ROLLOUT_KERNELS[rc]


def _rollout_outputs(R, t_max, dev):
    """actions [R, t_max] i64, logps [R, t_max] f32 and flags int32[4] = (steps, status, bad0, bad1) as views of ONE
    zero-filled buffer (one fill launch instead of three)."""
    n = R * t_max
    buf = torch.zeros(n * 12 + 16, dtype=torch.uint8, device=dev)
    actions = buf[:n * 8].view(torch.int64).view(R, t_max)
    logps = buf[n * 8:n * 12].view(torch.float32).view(R, t_max)
    flags = buf[n * 12:].view(torch.int32)
    return actions, logps, flags


HEADS_CAPTURE_MAX_BYTES = int(os.environ.get("EAMRL_HEADS_CAPTURE_MAX_BYTES", 48 << 30))   # 5 - 11 GB at the POMO sizes
_heads_skip_logged = False


def _capture_heads(st, cache, cs, R, t_max, want_heads):
    """Training: a [R, t_max, E] buffer for the steps' glimpse outputs where the kernel chosen for this shape writes it
    (eamrl_state.heads_out; st.heads afterwards, None otherwise).  The backward allocates a second buffer of the same size
    (dheads), so the capture is taken only while twice its size fits into half of the free device memory and under
    EAMRL_HEADS_CAPTURE_MAX_BYTES; otherwise -- and if the allocation fails -- the backward recomputes the glimpse (logged
    once: it is a slower path, not an error)."""
    global _heads_skip_logged
    st.heads = st.heads_out = None
    if not want_heads or st.env_name == "sdvrp" or not _lib.load().eamrl_rollout_rng_native(ENVS[st.env_name], C.byref(cs), R):
        return          # (SDVRP: its re-evaluation recomputes the glimpse -- the dynamic embedding's terms are not in the capture)
    need = R * int(t_max) * cache.E * 4
    free = torch.cuda.mem_get_info(st.mask.device)[0] + torch.cuda.memory_reserved(st.mask.device) - torch.cuda.memory_allocated(st.mask.device)
    reason = None
    if need > HEADS_CAPTURE_MAX_BYTES:
        reason = f"{need / 2**30:.1f} GiB > EAMRL_HEADS_CAPTURE_MAX_BYTES"
    elif 2 * need > free // 2:
        reason = f"2 x {need / 2**30:.1f} GiB would take more than half of the {free / 2**30:.1f} GiB free"
    else:
        try:
            st.heads = st.heads_out = torch.empty(R, int(t_max), cache.E, dtype=torch.float32, device=st.mask.device)
        except torch.cuda.OutOfMemoryError:
            reason = f"allocation of {need / 2**30:.1f} GiB failed"
    if reason and not _heads_skip_logged:
        _heads_skip_logged = True
        logging.getLogger(__name__).warning(
            "rollout: glimpse outputs of the decode steps are not kept for the backward (%s); the re-evaluation recomputes "
            "them (logits backward 18 instead of 11 ms at 1024 x 100 x 100)", reason)


def rollout(st: RolloutState, cache: DecodeCache, mode="greedy", noise=None, given=None, clip=10.0, temp=1.0,
            t_max=None, top_k=0, top_p=0.0, seed=None, seed_dev=None, return_flags=False, want_heads=False, poly=None,
            eas_layer=None):
    """Whole decode loop in one launch.  -> (actions [R,t_max], logps [R,t_max], info int32[2] = (steps, status)).
    poly: the operands of a PolyNet pointer (`polynet_operands`, on the device): the rollout runs the PolyNet case of the
    start-sharing kernel (one launch per 128 rows of an instance), or raises where that is not built.
    eas_layer: the parameters of an EAS-Lay layer (`eas_layer_operands`: one residual layer per instance, on the device): the
    rollout runs the layer case of the start-sharing kernel, or raises NotImplementedError where that is not built.  With
    want_heads the pre-layer glimpse outputs are kept in st.heads (and the call raises if that buffer cannot be had).
    Sampling takes its Exp(1) noise from `noise` [R, T, M] or, with `seed` (XOR the device word `seed_dev`), from the counter-based
    generator -- in place where the kernel supports it (TSP multistart), else through a scratch tensor of the same draws.
    return_flags: info is int32[4] = (steps, status, 0, 0), the last two free for the caller's validity counters."""
    _validate_state(st, cache)
    R, M = st.R, st.M
    if t_max is None:
        t_max = env_spec.max_steps(st.env_name, M)
    if mode == "sampling" and noise is None and seed is None:
        raise ValueError("rollout: sampling needs `noise` or `seed`")
    filtering = bool(top_k or (0.0 < top_p < 1.0))
    ext = cs = None
    if poly is not None or eas_layer is not None:
        if filtering:
            raise NotImplementedError(f"{'PolyNet' if poly is not None else 'EAS-Lay'} rollout: top-k / top-p filtering is not built")
        cs = cache.struct()         # (the extension's shape is asked of the library before anything is allocated)
        ext = _polynet_struct(st, cache, cs, poly) if poly is not None else _eas_layer_rollout_struct(st, cache, cs, eas_layer)
    elif mode == "sampling" and noise is None and filtering:
        # the kernels that filter (register-resident FILT variant, streaming) read their noise from a tensor
        noise = exp1_noise(seed, R, int(t_max), M, st.mask.device, seed_dev)
    noise, given, t_max, t_given = _rollout_inputs(noise, given, t_max, st.env_name, R, M)
    return _rollout_launch(st, cache, cs, ext, mode, noise, given, t_given, clip, temp, t_max, top_k, top_p, seed, seed_dev,
                           return_flags, want_heads and not filtering)


def _rollout_inputs(noise, given, t_max, env_name, R, M):
    """(noise, given, t_max, env, R, M) -> (noise, given, t_max, t_given) of a whole-rollout call: a noise tensor [R, T, M] sets
    t_max = T; given actions [R, T'] set t_given = T' and, without noise on a depot env, bound t_max by it (a TSP tour has its
    fixed length either way)."""
    t_given = 0
    if noise is not None:
        _chk(noise, "noise", torch.float32)
        if noise.dim() != 3 or noise.shape[0] != R or noise.shape[2] != M:
            raise ValueError("noise must be [R, T, M]")
        t_max = noise.shape[1]
    if given is not None:
        _chk(given, "given actions", torch.int64)
        if given.dim() != 2 or given.shape[0] != R:
            raise ValueError("given actions must be [R, T]")
        t_given = given.shape[1]
        if noise is None and env_name != "tsp":
            t_max = min(t_max, t_given)
    return noise, given, int(t_max), t_given


def _rollout_launch(st, cache, cs, ext, mode, noise, given, t_given, clip, temp, t_max, top_k, top_p, seed, seed_dev, return_flags,
                    want_heads):
    """The one launch path of `rollout`: outputs, the optional capture of the glimpse outputs, the state struct and the C call --
    eamrl_am_rollout or, for sampling without a noise tensor, eamrl_am_rollout_seeded; with ext = an eamrl_polynet / eamrl_eas_layer
    struct their PolyNet / EAS-Lay counterparts.  cs: the cache struct if the caller has built it already, else None."""
    lib = _lib.load()
    R = st.R
    actions, logps, info = _rollout_outputs(R, t_max, st.mask.device)          # info: [steps, status, -, -]
    if cs is None:
        cs = cache.struct()
    poly = ext if isinstance(ext, _lib.PolyNet) else None
    if poly is not None:
        st.heads = st.heads_out = None              # (the PolyNet case does not capture)
    else:
        _capture_heads(st, cache, cs, R, t_max, want_heads)
        if ext is not None and want_heads and st.heads is None:
            raise RuntimeError("EAS-Lay rollout: the buffer for the steps' glimpse outputs could not be had (see the log); the "
                               "layer's backward has no path without it")
    ss = st.struct()
    st.heads_out = None
    seeded = mode == "sampling" and noise is None
    seed64 = _seed64(seed if seeded else 0)
    head = (ENVS[st.env_name], C.byref(cs), C.byref(ss)) + (() if ext is None else (C.byref(ext),))
    tensors = (R, MODES[mode], _ptr(noise), _ptr(given), t_given)
    tail = (float(clip), float(temp))
    outs = (t_max, _ptr(actions), _ptr(logps), C.c_void_p(info.data_ptr()), C.c_void_p(info.data_ptr() + 4),
            _stream(st.mask))
    if ext is not None and poly is None:
        name, args = "eamrl_am_rollout_eas_layer", head + tensors + (int(seeded), seed64, _ptr(seed_dev if seeded else None)) + tail + outs
    elif poly is not None:
        name, args = (("eamrl_am_rollout_polynet_seeded", head + (R, seed64, _ptr(seed_dev)) + tail + outs) if seeded else
                      ("eamrl_am_rollout_polynet", head + tensors + tail + outs))
    elif seeded:
        native = lib.eamrl_rollout_rng_native(ENVS[st.env_name], C.byref(cs), R)
        scratch = None if native else torch.empty(R, t_max, st.M, dtype=torch.float32, device=st.mask.device)
        name, args = "eamrl_am_rollout_seeded", head + (R, seed64, _ptr(seed_dev), _ptr(scratch)) + tail + outs
    else:
        name, args = "eamrl_am_rollout", head + tensors + tail + (int(top_k), float(top_p)) + outs
    _lib.check(getattr(lib, name)(*args), name)
    return actions, logps, (info if return_flags else info[:2])


# ------------------------------------------------------------------------------------------------------
# PolyNet (eamrl_polynet): weight constants of the pointer, and the rollout on them
# ------------------------------------------------------------------------------------------------------
POLY_LAYER_DIM = 256        # the P the kernel is built for


def pack_mfma_a(W):
    """Row-major [N, K] -> the "fragment order" of include/eamrl.h (eamrl_polynet): float 4 * ((T * (K / 16) + q) * 64 + l) + i
    holds W[16 T + l % 16, 16 q + 4 i + l // 16] -- what lane l of a wavefront feeds into four consecutive
    v_mfma_f32_16x16x4_f32 as the A operand of row tile T, read with one 16-byte load.  Plain indexing (any device)."""
    N, K = W.shape
    assert N % 16 == 0 and K % 16 == 0
    dev = W.device
    T, q = torch.arange(N // 16, device=dev)[:, None, None, None], torch.arange(K // 16, device=dev)[None, :, None, None]
    l, i = torch.arange(64, device=dev)[None, None, :, None], torch.arange(4, device=dev)[None, None, None, :]
    return W[16 * T + l % 16, 16 * q + 4 * i + l // 16].contiguous().reshape(-1)


def polynet_operands(Wout, W1, b1, W2, b2, binary_vectors):
    """The weight-only operands of eamrl_polynet from the pointer's parameters (PolyNetAttention, nn/attention.py:502-517):
    project_out / poly_layer_1[:, :E] / poly_layer_2 in fragment order and ctab[j] = W1[:, E:] z_j + b1 ([k, P], computed
    in float64 and rounded once).  Any device; no kernel is launched."""
    E = Wout.shape[0]
    P = W1.shape[0]
    Z = binary_vectors.detach().double()
    ctab = (Z @ W1.detach()[:, E:].double().t() + b1.detach().double()).float().contiguous()
    return {"Wout": pack_mfma_a(Wout.detach().float()), "W1": pack_mfma_a(W1.detach()[:, :E].float()), "ctab": ctab,
            "W2": pack_mfma_a(W2.detach().float()), "b2": b2.detach().float().contiguous().clone(), "k": int(Z.shape[0]), "P": int(P)}


def rollout_polynet_supported(env_name, cache, R) -> bool:
    """Whether `rollout(..., poly=)` serves this env / cache shape / row count (eamrl_rollout_polynet_supported; host only)."""
    cs = cache if isinstance(cache, _lib.Cache) else cache.struct()
    return bool(_lib.load().eamrl_rollout_polynet_supported(ENVS.get(env_name, -1), C.byref(cs), int(R)))


def _polynet_struct(st, cache, cs, poly):
    """eamrl_polynet of `rollout(..., poly=)`: the operands validated against the cache, the shape against the library."""
    for name in ("Wout", "W1", "ctab", "W2", "b2"):
        _chk(poly[name], f"poly[{name!r}]", torch.float32)
    E, k, P = cache.E, int(poly["k"]), int(poly["P"])
    if P != POLY_LAYER_DIM:
        raise NotImplementedError(f"PolyNet rollout: poly_layer_dim = {P}; the kernel is built for {POLY_LAYER_DIM}")
    if (poly["Wout"].numel(), poly["W1"].numel(), poly["W2"].numel(), poly["b2"].numel()) != (E * E, P * E, E * P, E) \
            or tuple(poly["ctab"].shape) != (k, P):
        raise ValueError("PolyNet rollout: operand shapes do not match the cache (ops.polynet_operands)")
    if not _lib.load().eamrl_rollout_polynet_supported(ENVS.get(st.env_name, -1), C.byref(cs), st.R):
        raise NotImplementedError(f"PolyNet rollout: env {st.env_name!r} with {st.M} nodes and {st.R // cache.B} rows per instance is "
                                  "not built: TSP / CVRP, at most 112 nodes, at least two rows per instance, embed_dim 128, 8 heads")
    ps = _lib.PolyNet()
    ps.Wout, ps.W1, ps.ctab, ps.W2, ps.b2 = (poly[n].data_ptr() for n in ("Wout", "W1", "ctab", "W2", "b2"))
    ps.L = cache.slot_ptr("L")
    ps.k, ps.P, ps.s_offset = k, P, 0
    return ps


# ------------------------------------------------------------------------------------------------------
# EAS-Lay (eamrl_eas_layer): one residual layer per instance inside the decode step
# ------------------------------------------------------------------------------------------------------
def _eas_layer_index(E, dev):
    """[E * E] int64: position in a row-major [E, E] matrix W (y = x W) of every float of its kernel layout -- the fragment
    order (pack_mfma_a) of W^T: float 4 * ((T * (E / 16) + q) * 64 + l) + i holds W[16 q + 4 i + l // 16, 16 T + l % 16]."""
    T, q = torch.arange(E // 16, device=dev)[:, None, None, None], torch.arange(E // 16, device=dev)[None, :, None, None]
    l, i = torch.arange(64, device=dev)[None, None, :, None], torch.arange(4, device=dev)[None, None, None, :]
    return ((16 * q + 4 * i + l // 16) * E + 16 * T + l % 16).reshape(-1)


def pack_eas_layer(W):
    """[N, E, E] (y = x W[b], the reference's EASLayerNet.W1 / W2) -> [N, E * E] in the layout of eamrl_eas_layer.  Plain
    indexing (any device); `unpack_eas_layer` is its exact inverse."""
    N, E, E2 = W.shape
    assert E == E2 and E % 16 == 0
    return W.reshape(N, E * E)[:, _eas_layer_index(E, W.device)].contiguous()


def unpack_eas_layer(P, E=128):
    """[N, E * E] in the layout of eamrl_eas_layer -> [N, E, E] row-major (parameters and gradients alike)."""
    N = P.shape[0]
    out = torch.empty_like(P)
    out[:, _eas_layer_index(E, P.device)] = P
    return out.view(N, E, E)


def eas_layer_operands(W1, b1, W2, b2, forced=None):
    """The dict `rollout(..., eas_layer=)` and `ReevalPlan.backward_layer` take, from the reference's shapes: W1, W2 [N, E, E],
    b1, b2 [N, 1, E] or [N, E]; forced [N, t] int64 (optional: the tour of every instance's last row)."""
    N, E, _ = W1.shape
    d = {"W1": pack_eas_layer(W1.detach().float()), "b1": b1.detach().float().reshape(N, E).contiguous().clone(),
         "W2": pack_eas_layer(W2.detach().float()), "b2": b2.detach().float().reshape(N, E).contiguous().clone()}
    if forced is not None:
        d["forced"] = forced
    return d


def rollout_eas_layer_supported(env_name, cache, R) -> bool:
    """Whether `rollout(..., eas_layer=)` serves this env / cache shape / row count (eamrl_rollout_eas_layer_supported; host only)."""
    cs = cache if isinstance(cache, _lib.Cache) else cache.struct()
    return bool(_lib.load().eamrl_rollout_eas_layer_supported(ENVS.get(env_name, -1), C.byref(cs), int(R)))


def _eas_layer_struct(layer, B, E):
    for name, n in (("W1", E * E), ("b1", E), ("W2", E * E), ("b2", E)):
        _chk(layer[name], f"eas_layer[{name!r}]", torch.float32)
        if layer[name].numel() != B * n:
            raise ValueError(f"EAS-Lay: eas_layer[{name!r}] must hold {B} x {n} floats (one layer per instance: ops.eas_layer_operands)")
    ls = _lib.EasLayer()
    ls.W1, ls.b1, ls.W2, ls.b2 = (layer[n].data_ptr() for n in ("W1", "b1", "W2", "b2"))
    return ls


def _eas_layer_rollout_struct(st, cache, cs, layer):
    """eamrl_eas_layer of `rollout(..., eas_layer=)`: the shape checked against the library, the layer and `forced` against the cache."""
    if not _lib.load().eamrl_rollout_eas_layer_supported(ENVS.get(st.env_name, -1), C.byref(cs), st.R):
        raise NotImplementedError(f"EAS-Lay rollout: env {st.env_name!r} with {st.M} nodes and {st.R // cache.B} rows per instance is "
                                  f"not built: TSP / CVRP, 2 .. {KEY_CHUNK} nodes, 2 .. 128 rows per instance, embed_dim 128, 8 heads")
    ls = _eas_layer_struct(layer, cache.B, cache.E)
    forced = layer.get("forced")
    if forced is not None:
        _chk(forced, "eas_layer['forced']", torch.int64)
        if forced.dim() != 2 or forced.shape[0] != cache.B or forced.shape[1] < 1:
            raise ValueError("EAS-Lay: forced must be [B, t >= 1] int64")
        ls.forced, ls.t_forced = forced.data_ptr(), forced.shape[1]
    return ls


def raise_on_status(status: int):
    """The reference's in-loop asserts, checked once per rollout instead of once per step."""
    if status & ST_NAN_LOGITS:
        raise AssertionError("Logits contain NaNs")                       # nn/attention.py:303-304
    if status & ST_INFEASIBLE:
        raise AssertionError("infeasible action selected")               # utils/decoding.py:397-399


# ------------------------------------------------------------------------------------------------------
# Pointer Network (csrc/ptrnet.hip)
# ------------------------------------------------------------------------------------------------------
PTRNET_WEIGHTS = {     # eamrl_ptrnet field -> (state-dict key, shape)
    "embedding": ("embedding", (2, 128)), "dec_in0": ("decoder_in_0", (128,)),
    "enc_w_ih": ("encoder.lstm.weight_ih_l0", (512, 128)), "enc_w_hh": ("encoder.lstm.weight_hh_l0", (512, 128)),
    "enc_b_ih": ("encoder.lstm.bias_ih_l0", (512,)), "enc_b_hh": ("encoder.lstm.bias_hh_l0", (512,)),
    "dec_w_ih": ("decoder.lstm.weight_ih", (512, 128)), "dec_w_hh": ("decoder.lstm.weight_hh", (512, 128)),
    "dec_b_ih": ("decoder.lstm.bias_ih", (512,)), "dec_b_hh": ("decoder.lstm.bias_hh", (512,)),
    "g_v": ("decoder.glimpse.v", (128,)), "g_wq": ("decoder.glimpse.project_query.weight", (128, 128)),
    "g_bq": ("decoder.glimpse.project_query.bias", (128,)),
    "p_v": ("decoder.pointer.v", (128,)), "p_wq": ("decoder.pointer.project_query.weight", (128, 128)),
    "p_bq": ("decoder.pointer.project_query.bias", (128,)),
}
PTRNET_MAX_NODES = 128


def _ptrnet_struct(locs, weights, clip):
    """(struct, keep-alive list): eamrl_ptrnet over `locs` [B, N, 2] and `weights` (state-dict key -> fp32 device tensor)."""
    _chk(locs, "locs", torch.float32)
    if locs.dim() != 3 or locs.shape[2] != 2:
        raise ValueError(f"ptrnet: locs must be [B, N, 2], got {tuple(locs.shape)}")
    B, N, _ = locs.shape
    if not 2 <= N <= PTRNET_MAX_NODES:
        raise NotImplementedError(f"ptrnet: graphs of 2..{PTRNET_MAX_NODES} nodes are built, got {N}")
    s = _lib.PtrNet()
    keep = [locs]
    s.locs = _ptr(locs)
    for field, (key, shape) in PTRNET_WEIGHTS.items():
        t = _chk(weights[key], key, torch.float32, shape)
        keep.append(t)
        setattr(s, field, _ptr(t))
    s.B, s.N, s.E, s.H, s.clip = B, N, 128, 128, float(clip)
    return s, keep


def ptrnet_encode(locs, weights, ws=None):
    """The Pointer Network encoder (eamrl_ptrnet_encode): nn.LSTM over the nodes 0..N-1 of x_n = locs_n @ embedding from the
    zero state, all N steps in one launch.  -> ctx [B, N, 128], h [B, 128], c [B, 128], ws (the scratch the rollout call
    takes again)."""
    lib = _lib.load()
    s, keep = _ptrnet_struct(locs, weights, 1.0)
    B, N, _ = locs.shape
    dev = locs.device
    ctx = torch.empty(B, N, 128, device=dev, dtype=torch.float32)
    h = torch.empty(B, 128, device=dev, dtype=torch.float32)
    c = torch.empty(B, 128, device=dev, dtype=torch.float32)
    ws = torch.empty(_lib.PTRNET_WS_FLOATS, device=dev, dtype=torch.float32) if ws is None else ws
    s.ctx, s.h, s.c, s.ws = _ptr(ctx), _ptr(h), _ptr(c), _ptr(ws)
    _lib.check(lib.eamrl_ptrnet_encode(C.byref(s), _stream(locs)), "eamrl_ptrnet_encode")
    return ctx, h, c, ws


def ptrnet_rollout(locs, weights, h, c, e_g, e_p, clip=10.0, mode="greedy", noise=None, given=None, seed=None, ws=None):
    """The Pointer Network decode loop (eamrl_ptrnet_rollout[_seeded]), all N steps in one launch.  h, c: the encoder's final
    state; e_g, e_p [B, N, 128]: project_ref of the glimpse / the pointer applied to ctx.  mode "sampling" takes noise
    [B, N, N] (Exp(1) draws, [instance][step][node]) or a seed (the draws of exp1_noise(seed, B, N, N)); "evaluate" takes
    given [B, N].  -> actions [B, N] int64, logp [B, N] (the chosen node's log-probability per step)."""
    lib = _lib.load()
    s, keep = _ptrnet_struct(locs, weights, clip)
    B, N, _ = locs.shape
    dev = locs.device
    _chk(h, "h", torch.float32, (B, 128)), _chk(c, "c", torch.float32, (B, 128))
    _chk(e_g, "e_g", torch.float32, (B, N, 128)), _chk(e_p, "e_p", torch.float32, (B, N, 128))
    m = MODES[mode]
    if m == SAMPLE and (noise is None) == (seed is None):
        raise ValueError("ptrnet_rollout(mode='sampling') takes exactly one of noise= and seed=")
    if m == SAMPLE and noise is not None:
        _chk(noise, "noise", torch.float32, (B, N, N))
    if m == EVALUATE:
        if given is None:
            raise ValueError("ptrnet_rollout(mode='evaluate') needs given=")
        _chk(given, "given", torch.int64, (B, N))
    ws = torch.empty(_lib.PTRNET_WS_FLOATS, device=dev, dtype=torch.float32) if ws is None else ws
    actions = torch.empty(B, N, device=dev, dtype=torch.int64)
    logp = torch.empty(B, N, device=dev, dtype=torch.float32)
    s.h, s.c, s.e_g, s.e_p, s.ws = _ptr(h), _ptr(c), _ptr(e_g), _ptr(e_p), _ptr(ws)
    if m == SAMPLE and noise is None:
        _lib.check(lib.eamrl_ptrnet_rollout_seeded(C.byref(s), _seed64(seed), _ptr(actions), _ptr(logp), _stream(locs)),
                   "eamrl_ptrnet_rollout_seeded")
    else:
        _lib.check(lib.eamrl_ptrnet_rollout(C.byref(s), m, _ptr(noise) if m == SAMPLE else None,
                                            _ptr(given) if m == EVALUATE else None, _ptr(actions), _ptr(logp), _stream(locs)),
                   "eamrl_ptrnet_rollout")
    return actions, logp
