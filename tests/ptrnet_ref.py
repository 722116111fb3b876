"""Plain-torch restatement of the Pointer Network (encoder LSTM + decode loop) on a dict of weights keyed like the reference's
state dict; runs in the dtype of the weights (float64 or float32) on any device.  Independent of eam_rl4co_amd: the tests pin
it to the reference's recorded float64 log-probs first (test_host_ptrnet.py) and the kernels to it afterwards.

`mutant=` breaks one rule on purpose; every mutant must miss the fixtures by far more than the float32 error:
    "gate_order"       gates read as i, g, f, o
    "no_bhh"           the recurrent biases dropped
    "glimpse_unmasked" visited nodes take part in the glimpse softmax
    "raw_readout"      the glimpse reads out the encoder outputs instead of the projected refs
"""
import math

import torch

MUTANTS = ("gate_order", "no_bhh", "glimpse_unmasked", "raw_readout")


def closed_form_weights(shapes, dtype=torch.float32):
    """p_k[i] = 3 / sqrt(fan_in) * sin(i * (0.37 + 0.11 k) + k) for the k-th entry of `shapes` (an ordered key -> shape mapping,
    the state dict's order), i the flat index; fan_in = 2 for `embedding`, the input width of a matrix, 128 for a vector.
    Evaluated in float64 and rounded once to float32 (the values every precision then shares), returned as `dtype`.
    The default initialisation gives near-uniform distributions (exact greedy ties from N = 50 on); these are peaky."""
    out = {}
    for k, (key, shape) in enumerate(shapes.items()):
        shape = tuple(shape)
        fan_in = 2 if key == "embedding" else (shape[1] if len(shape) >= 2 else 128)
        i = torch.arange(math.prod(shape), dtype=torch.float64)
        p = 3.0 / math.sqrt(fan_in) * torch.sin(i * (0.37 + 0.11 * k) + k)
        out[key] = p.reshape(shape).to(torch.float32).to(dtype)
    return out


def _cell(xg, h, c, w_hh, b_hh, mutant):
    gates = xg + h @ w_hh.T
    if mutant != "no_bhh":
        gates = gates + b_hh
    if mutant == "gate_order":
        i, g, f, o = gates.chunk(4, dim=1)
    else:
        i, f, g, o = gates.chunk(4, dim=1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def rollout(w, locs, mode="greedy", given=None, noise=None, clip=10.0, mutant=None):
    """-> actions [B, N] int64, logp [B, N] (chosen node per step), gap [B]: the smallest (best - second best) decision margin of
    the row over its steps, of the log-probs (greedy) or of log-prob - log(noise) (sampling); inf for mode="evaluate"."""
    assert mutant is None or mutant in MUTANTS
    dt = w["embedding"].dtype
    locs = locs.to(dt)
    B, N, _ = locs.shape
    x = locs @ w["embedding"]
    h = c = locs.new_zeros(B, 128)
    xg = x @ w["encoder.lstm.weight_ih_l0"].T + w["encoder.lstm.bias_ih_l0"]
    ctx = []
    for n in range(N):
        h, c = _cell(xg[:, n], h, c, w["encoder.lstm.weight_hh_l0"], w["encoder.lstm.bias_hh_l0"], mutant)
        ctx.append(h)
    ctx = torch.stack(ctx, 1)
    G, P = "decoder.glimpse.", "decoder.pointer."
    e_g = ctx @ w[G + "project_ref.weight"][:, :, 0].T + w[G + "project_ref.bias"]
    e_p = ctx @ w[P + "project_ref.weight"][:, :, 0].T + w[P + "project_ref.bias"]
    dg = x @ w["decoder.lstm.weight_ih"].T + w["decoder.lstm.bias_ih"]
    din = (w["decoder.lstm.weight_ih"] @ w["decoder_in_0"] + w["decoder.lstm.bias_ih"]).expand(B, -1)
    visited = torch.zeros(B, N, dtype=torch.bool, device=locs.device)
    gap = torch.full((B,), float("inf"), dtype=torch.float64, device=locs.device)
    acts, lps = [], []
    for t in range(N):
        h, c = _cell(din, h, c, w["decoder.lstm.weight_hh"], w["decoder.lstm.bias_hh"], mutant)
        q = h @ w[G + "project_query.weight"].T + w[G + "project_query.bias"]
        u = (torch.tanh(q[:, None, :] + e_g) * w[G + "v"]).sum(-1)
        if mutant != "glimpse_unmasked":
            u = u.masked_fill(visited, float("-inf"))
        p = torch.softmax(u, dim=1)
        g = (p[:, :, None] * (ctx if mutant == "raw_readout" else e_g)).sum(1)
        q = g @ w[P + "project_query.weight"].T + w[P + "project_query.bias"]
        u = (torch.tanh(q[:, None, :] + e_p) * w[P + "v"]).sum(-1)
        lp = torch.log_softmax((clip * torch.tanh(u)).masked_fill(visited, float("-inf")), dim=1)
        if mode == "evaluate":
            sel = given[:, t]
        else:
            key = lp.double()
            if mode == "sampling":
                key = key - noise[:, t].double().log()
            sel = key.argmax(1)
            if N - t >= 2:
                top = torch.topk(key, 2, dim=1).values
                gap = torch.minimum(gap, top[:, 0] - top[:, 1])
        acts.append(sel)
        lps.append(lp.gather(1, sel[:, None]).squeeze(1))
        visited = visited.scatter(1, sel[:, None], True)
        din = dg.gather(1, sel[:, None, None].expand(B, 1, 512)).squeeze(1)
    return torch.stack(acts, 1), torch.stack(lps, 1), gap
