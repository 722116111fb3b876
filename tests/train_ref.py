"""Plain restatements of the operations behind the differentiable encoder (eam_rl4co_amd/train.py: _LinearFn, _SmallLinearFn,
_InstanceNormFn, _BatchNormTrainFn, _self_attention), in torch on the CPU.  Nothing here comes from the package.

Written from the definitions -- torch.nn.Linear's weight / bias gradient, InstanceNorm1d(affine) over the nodes of [B, N, E],
BatchNorm1d with batch statistics over the rows of [rows, E], softmax self-attention on qkv packed "b s (three h d)" -- with the
formulas the kernels' header comments state:

    xhat = (x - mean) rstd,  rstd = 1 / sqrt(var + eps),  var = mean((x - mean)^2)   (two passes, biased)
    y = xhat gamma + beta
    dx = gamma rstd (dy - mean(dy) - xhat mean(dy xhat)),  dgamma = sum dy xhat,  dbeta = sum dy

Every function computes in `dtype`: float64 is the reference, the float32 run gives the scale of float32 rounding
(tests/train_cases.py).  The sums are torch's own (`sum`, `mean`, `@`): their order is not the kernels'.
"""
import math

import torch


def linear_wgrad(dy, x, dtype=torch.float64):
    """dy [rows, out], x [rows, in] -> dW [out, in] = dy^T x, db [out] = the column sums of dy."""
    dy, x = dy.to(dtype), x.to(dtype)
    return dy.t() @ x, dy.sum(0)


def small_linear_wgrad(dy, x, dtype=torch.float64):
    """The same for a Linear with K <= 8 inputs: dy [rows, out], x [rows, K] -> dW [out, K], db [out]."""
    dy, x = dy.to(dtype), x.to(dtype)
    return dy.t() @ x, dy.sum(0)


def instance_norm(x, gamma, beta, eps, dy, dtype=torch.float64, one_pass=False):
    """x, dy [B, N, E]; gamma, beta [E] -> y [B, N, E], mean, rstd [B, E], dx [B, N, E], dgamma, dbeta [E].
    `one_pass`: the variance as mean(x^2) - mean(x)^2 (the deliberately wrong form of tests/test_host_train_ref.py)."""
    x, gamma, beta, dy = (t.to(dtype) for t in (x, gamma, beta, dy))
    mean = x.mean(1)
    d = x - mean[:, None]
    var = ((x * x).mean(1) - mean * mean).clamp_min(0) if one_pass else (d * d).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = d * rstd[:, None]
    y = xhat * gamma + beta
    m1, m2 = dy.mean(1), (dy * xhat).mean(1)
    dx = (gamma * rstd)[:, None] * (dy - m1[:, None] - xhat * m2[:, None])
    return y, mean, rstd, dx, (dy * xhat).sum((0, 1)), dy.sum((0, 1))


def batchnorm_backward(x, dy, gamma, eps, dtype=torch.float64, stats=None):
    """x, dy [rows, E]; gamma [E] -> mean, var [E] (biased), dx [rows, E], dgamma, dbeta [E].
    `stats` = (mean, var) given instead of computed: the kernel takes them as operands (the forward pass kept them)."""
    x, gamma, dy = (t.to(dtype) for t in (x, gamma, dy))
    if stats is None:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
    else:
        mean, var = (t.to(dtype) for t in stats)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    dbeta, dgamma = dy.sum(0), (dy * xhat).sum(0)
    n = x.shape[0]
    dx = gamma * rstd * (dy - dbeta / n - xhat * (dgamma / n))
    return mean, var, dx, dgamma, dbeta


def attention_backward(qkv, dout, H, dtype=torch.float64, keys=None, skip_queries=None):
    """qkv [B, N, 3E] packed q | k | v with H heads each, dout [B, N, E] -> y [B, N, E], dqkv [B, N, 3E].
    p = softmax(q k^T / sqrt(D)) over the keys, y = p v;  dv = p^T dout,  dp = dout v^T,  ds = p (dp - sum p dp),
    dq = ds k / sqrt(D),  dk = ds^T q / sqrt(D).  Two deliberately wrong forms, for the planted errors of the tests: `keys`: only the
    first `keys` nodes are attended to (a bool tensor [N]: only the nodes it marks);  `skip_queries` (indices): these query rows are
    left out of the sums over the queries, dk and dv (y and dq are as without it)."""
    qkv, dout = qkv.to(dtype), dout.to(dtype)
    B, N, E3 = qkv.shape
    E = E3 // 3
    D = E // H
    q, k, v = (qkv[..., i * E:(i + 1) * E].reshape(B, N, H, D).permute(0, 2, 1, 3) for i in range(3))      # [B, H, N, D]
    do = dout.reshape(B, N, H, D).permute(0, 2, 1, 3)
    s = q @ k.transpose(-1, -2) / math.sqrt(D)
    if isinstance(keys, torch.Tensor):
        s[..., ~keys] = -math.inf
    elif keys is not None:
        s[..., keys:] = -math.inf
    p = torch.softmax(s, dim=-1)
    y = p @ v
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    dq = ds @ k / math.sqrt(D)
    if skip_queries is not None:
        p, ds = p.clone(), ds.clone()
        p[..., skip_queries, :] = 0
        ds[..., skip_queries, :] = 0
    dv = p.transpose(-1, -2) @ do
    dk = ds.transpose(-1, -2) @ q / math.sqrt(D)
    flat = (lambda t: t.permute(0, 2, 1, 3).reshape(B, N, E))
    return flat(y), torch.cat([flat(dq), flat(dk), flat(dv)], dim=-1)
