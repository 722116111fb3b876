"""Torch CPU restatement of the Heterogeneous Attention Model's encoder attention (rl4co/models/zoo/ham/attention.py,
Li et al. 2021) and of the encoder around it, with a `dtype` argument.  Imports nothing from the package under test.

Nodes: depot 0, pickups 1..P, deliveries P+1..2P, M = 2P + 1; the partner of pickup i is i + P, of delivery i it is i - P.
H heads of width D = E / H, c = 1 / sqrt(D).  `proj` [B, M, 6E] = q | k | v | qpair | qsame | qother, each "(h d)": all nodes
take q, k, v from W_query, W_key, W_val; a pickup takes the three extra queries from W1, W2, W3, a delivery from W4, W5, W6 (the
depot's last 3E are ignored).  Scores per head and row i:
  general  c q_i k_j for all j;   pair  c qpair_i k_partner(i);   same  c qsame_i k_j, j of i's role;   other  c qother_i k_j, j of
  the opposite role.
The depot row has the M general scores only; a non-depot row has 2M scores under ONE softmax, and because every group uses the
same k and v:   out_i = sum_j (a_gen + a_same + a_other)[i, j] v_j + a_pair[i] v_partner(i).

`wrong=` gives deliberately wrong forms, for the tests that show the fixtures can tell them apart:
  "no_pair"   the pair term dropped;   "swapped"  same and other exchanged;   "separate"  every group under a softmax of its own.
"""
import math

import torch

WRONG = ("no_pair", "swapped", "separate")
NEG = float("-inf")


def _scores(proj, H, wrong=None):
    """-> (s_gen [B,H,M,M], s_x [B,H,M,M], s_pair [B,H,M], v [B,H,M,D], partner [M]); -inf where a group has no score."""
    B, M, E6 = proj.shape
    assert M % 2 == 1, "Graph size should have odd number of nodes"
    E = E6 // 6
    D = E // H
    P = (M - 1) // 2
    c = 1.0 / math.sqrt(D)
    q, k, v, qp, qs, qo = (proj[..., i * E:(i + 1) * E].reshape(B, M, H, D).permute(0, 2, 1, 3) for i in range(6))
    if wrong == "swapped":
        qs, qo = qo, qs
    role = torch.zeros(M, dtype=torch.long)
    role[1:P + 1], role[P + 1:] = 1, 2
    idx = torch.arange(M)
    partner = torch.where(role == 1, idx + P, torch.where(role == 2, idx - P, idx))
    nd = role != 0
    s_gen = c * (q @ k.transpose(-1, -2))
    pair_ok = nd
    s_pair = torch.where(pair_ok, c * (qp * k[:, :, partner]).sum(-1), torch.full((), NEG, dtype=proj.dtype))
    live = nd[:, None] & nd[None, :]
    same = role[:, None] == role[None, :]
    # the depot's extra queries are never used: zero them so that garbage there cannot reach the result through 0 * nan
    qs = torch.where(nd[:, None], qs, torch.zeros((), dtype=proj.dtype))
    qo = torch.where(nd[:, None], qo, torch.zeros((), dtype=proj.dtype))
    s_x = torch.where(same, c * (qs @ k.transpose(-1, -2)), c * (qo @ k.transpose(-1, -2)))
    s_x = torch.where(live, s_x, torch.full((), NEG, dtype=proj.dtype))
    if wrong == "no_pair":
        s_pair = torch.full_like(s_pair, NEG)
    return s_gen, s_x, s_pair, v, partner, live, same


def hetero_mha(proj, H, dtype=torch.float64, wrong=None):
    """proj [B, M, 6E] -> the heads [B, M, E] "(h d)" before W_out."""
    assert wrong is None or wrong in WRONG
    proj = proj.to(dtype)
    B, M, E6 = proj.shape
    s_gen, s_x, s_pair, v, partner, live, same = _scores(proj, H, wrong)
    if wrong == "separate":
        a_gen = torch.softmax(s_gen, -1)
        a_pair = torch.where(torch.isfinite(s_pair), torch.ones_like(s_pair), torch.zeros_like(s_pair))
        neg = torch.full((), NEG, dtype=dtype)
        a_x = torch.zeros_like(s_x)
        for grp in (live & same, live & ~same):
            a = torch.softmax(torch.where(grp, s_x, neg), -1)
            a_x = a_x + torch.where(grp, a, torch.zeros((), dtype=dtype))       # (rows without the group: softmax of all -inf is nan)
    else:
        allsc = torch.cat((s_gen, s_x, s_pair[..., None]), -1)
        a = torch.softmax(allsc, -1)
        a_gen, a_x, a_pair = a[..., :M], a[..., M:2 * M], a[..., 2 * M]
    heads = (a_gen + a_x) @ v + a_pair[..., None] * v[:, :, partner]
    return heads.permute(0, 2, 1, 3).reshape(B, M, E6 // 6)


def hetero_mha_backward(proj, dout, H, dtype=torch.float64):
    """-> (out [B, M, E], dproj [B, M, 6E]) of hetero_mha for the output gradient dout; the depot's last 3E of dproj are zeros."""
    p = proj.to(dtype).clone().requires_grad_(True)
    out = hetero_mha(p, H, dtype)
    (g,) = torch.autograd.grad(out, p, dout.to(dtype))
    return out.detach(), g


QUERY_KEYS = ("W_query", "W_key", "W_val")
PICK_KEYS = ("W1_query", "W2_query", "W3_query")
DELIV_KEYS = ("W4_query", "W5_query", "W6_query")
WEIGHT_KEYS = QUERY_KEYS + PICK_KEYS + DELIV_KEYS + ("W_out",)


def project(x, w, dtype=torch.float64):
    """x [B, M, E] and the module's weights {name: [H, E, D]} -> proj [B, M, 6E]."""
    x = x.to(dtype)
    B, M, E = x.shape
    P = (M - 1) // 2
    flat = lambda name: w[name].to(dtype).permute(1, 0, 2).reshape(E, -1)        # [E, (h d)]
    qkv = torch.cat([x @ flat(n) for n in QUERY_KEYS], -1)
    pick = torch.cat([x[:, 1:P + 1] @ flat(n) for n in PICK_KEYS], -1)
    deliv = torch.cat([x[:, P + 1:] @ flat(n) for n in DELIV_KEYS], -1)
    extra = torch.cat((torch.zeros(B, 1, pick.shape[-1], dtype=dtype), pick, deliv), 1)
    return torch.cat((qkv, extra), -1)


def module_forward(x, w, dtype=torch.float64, wrong=None):
    """HeterogenousMHA.forward(x) for the weights w (WEIGHT_KEYS): projections, attention, W_out."""
    H, E, D = w["W_query"].shape
    heads = hetero_mha(project(x, w, dtype), H, dtype, wrong)
    return heads @ w["W_out"].to(dtype).reshape(H * D, -1)


def _norm(h, sd, prefix, kind, eps=1e-5):
    g, b = sd[prefix + "weight"], sd[prefix + "bias"]
    if kind == "batch":     # eval mode: the running statistics
        mean, var = sd[prefix + "running_mean"], sd[prefix + "running_var"]
        return (h - mean) / torch.sqrt(var + eps) * g + b
    mean = h.mean(1, keepdim=True)
    var = ((h - mean) ** 2).mean(1, keepdim=True)
    return (h - mean) / torch.sqrt(var + eps) * g + b


def pdp_init_embedding(locs, sd, dtype=torch.float64, prefix="encoder.init_embedding."):
    locs = locs.to(dtype)
    P = (locs.shape[1] - 1) // 2
    lin = lambda x, n: x @ sd[prefix + n + ".weight"].to(dtype).t() + sd[prefix + n + ".bias"].to(dtype)
    pick, deliv = locs[:, 1:P + 1], locs[:, P + 1:]
    return torch.cat((lin(locs[:, :1], "init_embed_depot"), lin(torch.cat((pick, deliv), -1), "init_embed_pick"),
                      lin(deliv, "init_embed_delivery")), 1)


def encoder(locs, sd, num_layers, normalization, dtype=torch.float64):
    """GraphHeterogeneousAttentionEncoder.forward in eval mode for the policy state dict sd -> (embeddings, init embeddings)."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    init = pdp_init_embedding(locs, sd, dtype)
    h = init
    for l in range(num_layers):
        pre = f"encoder.layers.{l}."
        w = {n: sd[pre + "0.module." + n] for n in WEIGHT_KEYS}
        h = _norm(h + module_forward(h, w, dtype), sd, pre + "1.normalizer.", normalization)
        ff = torch.relu(h @ sd[pre + "2.module.0.weight"].t() + sd[pre + "2.module.0.bias"])
        ff = ff @ sd[pre + "2.module.2.weight"].t() + sd[pre + "2.module.2.bias"]
        h = _norm(h + ff, sd, pre + "3.normalizer.", normalization)
    return h, init
