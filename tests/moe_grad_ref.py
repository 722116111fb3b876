"""The experts of the MoE sublayer with the routing GIVEN, and their gradients, as a float64 statement on the CPU: the
formula of include/eamrl.h (eamrl_moe_experts_forward / _backward) written out row list by row list -- no autograd, no
reference program text.

    o[row, j]  = b2_e + W2_e relu(b1_e + W1_e x[row]),  e = sel[row, j]
    y[row]     = sum over the row's slots in ascending expert index of g[row, j] * o[row, j]
    dg[row, j] = <dy[row], o[row, j]>
    per expert e over its rows:  dO = g * dy,  dHid = (dO W2_e) * [hid > 0],  dW2_e = dO^T hid,  db2_e = sum dO,
                                 dW1_e = dHid^T x,  db1_e = sum dHid
    dx[row]    = sum over the row's slots of dHid W1_e
"""
import numpy as np
import torch


def experts_grad_ref(x, sel, g, W1, b1, W2, b2, dy):
    """x [rows, 128], sel [rows, k] integers, g [rows, k], W1 [n, 512, 128], b1 [n, 512], W2 [n, 128, 512], b2 [n, 128],
    dy [rows, 128] (numpy or torch, any float dtype) -> dict of float64 numpy arrays y, o, dx, dg, dW1, db1, dW2, db2."""
    x, g, W1, b1, W2, b2, dy = (torch.as_tensor(np.asarray(v), dtype=torch.float64) for v in (x, g, W1, b1, W2, b2, dy))
    sel = torch.as_tensor(np.asarray(sel)).long()
    rows, k = sel.shape
    n = W1.shape[0]
    y, dx = torch.zeros_like(x), torch.zeros_like(x)
    o = torch.zeros(rows, k, x.shape[1], dtype=torch.float64)
    dg = torch.zeros(rows, k, dtype=torch.float64)
    dW1, db1, dW2, db2 = torch.zeros_like(W1), torch.zeros_like(b1), torch.zeros_like(W2), torch.zeros_like(b2)
    for e in range(n):
        r, j = torch.nonzero(sel == e, as_tuple=True)
        if r.numel() == 0:
            continue
        xe = x[r]
        pre = xe @ W1[e].t() + b1[e]
        hid = torch.relu(pre)
        oe = hid @ W2[e].t() + b2[e]
        o[r, j] = oe
        y[r] += g[r, j, None] * oe
        dg[r, j] = (dy[r] * oe).sum(1)
        dO = g[r, j, None] * dy[r]
        dHid = (dO @ W2[e]) * (pre > 0)
        dW2[e], db2[e] = dO.t() @ hid, dO.sum(0)
        dW1[e], db1[e] = dHid.t() @ xe, dHid.sum(0)
        dx[r] += dHid @ W1[e]
    return {k_: v.numpy() for k_, v in dict(y=y, o=o, dx=dx, dg=dg, dW1=dW1, db1=db1, dW2=dW2, db2=db2).items()}


def make_case(rows, n_exp, k, seed, routing="random"):
    """Seeded inputs with an explicit routing (float32 arrays).  routing: "random" -- every row draws k distinct experts;
    "skip_last" -- the last expert receives no row (k < n_exp); "all_on_0" -- every row's first slot is expert 0;
    or a tuple of per-expert counts for k = 1 (rows = their sum), dealt in a shuffled row order."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    x = rng.standard_normal((rows, 128)).astype(f32)
    dy = rng.standard_normal((rows, 128)).astype(f32)
    W1 = (rng.uniform(-1, 1, (n_exp, 512, 128)) / np.sqrt(128)).astype(f32)
    b1 = rng.uniform(-0.1, 0.1, (n_exp, 512)).astype(f32)
    W2 = (rng.uniform(-1, 1, (n_exp, 128, 512)) / np.sqrt(512)).astype(f32)
    b2 = rng.uniform(-0.1, 0.1, (n_exp, 128)).astype(f32)
    if isinstance(routing, tuple):
        assert k == 1 and sum(routing) == rows and len(routing) == n_exp
        sel = rng.permutation(np.repeat(np.arange(n_exp), routing))[:, None].astype(np.int8)
    else:
        pool = n_exp - 1 if routing == "skip_last" else n_exp
        assert k <= pool
        sel = np.stack([rng.permutation(pool)[:k] for _ in range(rows)]).astype(np.int8)
        if routing == "all_on_0":
            for r in range(rows):
                if 0 not in sel[r]:
                    sel[r, 0] = 0
    g = rng.uniform(0.1, 1.0, (rows, k)).astype(f32)
    g = (g / (g.sum(1, keepdims=True) + f32(1e-6))).astype(f32)
    return dict(x=x, sel=sel, g=g, W1=W1, b1=b1, W2=W2, b2=b2, dy=dy)
