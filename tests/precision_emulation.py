"""The 16-bit encoder contract ("16-bit encoder") restated in float64 numpy, rounding to T at exactly the
contract's points, for comparison with eamrl_encoder_fused16.  With `rnd=None` nothing is rounded and the emulation is
the fp32 encoder + cache of the oracle in float64."""
import numpy as np


def round_bf16(x):
    """float64 -> fp32 -> bf16 (round to nearest even, NaN kept) -> float64."""
    f = np.ascontiguousarray(x, dtype=np.float32)
    b = f.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    out = r.view(np.float32).astype(np.float64)
    return np.where(np.isnan(f), np.nan, out)


def round_fp16(x):
    """float64 -> fp32 -> fp16 (round to nearest even) -> float64."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float64)


ROUNDING = {"bf16": round_bf16, "fp16": round_fp16}


def _id(x):
    return np.asarray(x, dtype=np.float64)


def _linear(x, W, b, rnd):
    """Node Linear: both operands rounded, fp32 (here float64) accumulation, fp32 bias."""
    y = rnd(x) @ rnd(np.asarray(W, np.float64)).T
    return y if b is None else y + np.asarray(b, np.float64)


def _attention(qkv, H, rnd):
    B, N, E3 = qkv.shape
    E = E3 // 3
    D = E // H
    q = rnd(qkv[..., :E] * 0.25).reshape(B, N, H, D).transpose(0, 2, 1, 3)
    k = rnd(qkv[..., E:2 * E]).reshape(B, N, H, D).transpose(0, 2, 1, 3)
    v = rnd(qkv[..., 2 * E:]).reshape(B, N, H, D).transpose(0, 2, 1, 3)
    s = q @ k.transpose(0, 1, 3, 2)
    w = rnd(np.exp(s - s.max(-1, keepdims=True)))
    o = (w @ v) / w.sum(-1, keepdims=True)
    return o.transpose(0, 2, 1, 3).reshape(B, N, E)


def _norm(sd, p, h):
    g, b = (np.asarray(sd[p + k], np.float64) for k in ("weight", "bias"))
    if p + "running_mean" in sd:
        m, v = (np.asarray(sd[p + k], np.float64) for k in ("running_mean", "running_var"))
        sc = g / np.sqrt(v + 1e-5)
        return h * sc + (b - m * sc)
    mean = h.mean(1, keepdims=True)
    var = ((h - mean) ** 2).mean(1, keepdims=True)
    return (h - mean) / np.sqrt(var + 1e-5) * g + b


def encode(sd, init_h, rnd=None, num_heads=8):
    """init embeddings [B, M, E] -> node embeddings (float64), eval-mode batch norm or instance norm."""
    rnd = rnd or _id
    h = np.asarray(init_h, np.float64)
    layer = 0
    while f"encoder.net.layers.{layer}.0.module.Wqkv.weight" in sd:
        p = f"encoder.net.layers.{layer}."
        qkv = _linear(h, sd[p + "0.module.Wqkv.weight"], sd[p + "0.module.Wqkv.bias"], rnd)
        att = _attention(qkv, num_heads, rnd)
        h = _norm(sd, p + "1.normalizer.", h + _linear(att, sd[p + "0.module.out_proj.weight"], sd[p + "0.module.out_proj.bias"], rnd))
        f = np.maximum(_linear(h, sd[p + "2.module.lins.0.weight"], sd[p + "2.module.lins.0.bias"], rnd), 0.0)
        h = _norm(sd, p + "3.normalizer.", h + _linear(f, sd[p + "2.module.lins.1.weight"], sd[p + "2.module.lins.1.bias"], rnd))
        layer += 1
    return h


def precompute(sd, env_name, emb, rnd=None, use_graph_context=True):
    """Decoder cache of the 16-bit path: K, V, L, Pa (, Pb), Lp = L Wout as node Linears, the graph context in fp32."""
    rnd = rnd or _id
    emb = np.asarray(emb, np.float64)
    E = emb.shape[-1]
    Wkvl = np.asarray(sd["decoder.project_node_embeddings.weight"], np.float64)
    Wctx = np.asarray(sd["decoder.context_embedding.project_context.weight"], np.float64)
    out = {n: _linear(emb, Wkvl[i * E:(i + 1) * E], None, rnd) for i, n in enumerate(("K", "V", "L"))}
    out["Pa"] = _linear(emb, Wctx[:, :E], None, rnd)
    out["Pb"] = _linear(emb, Wctx[:, E:2 * E], None, rnd) if env_name == "tsp" else None
    out["Lp"] = _linear(out["L"], np.asarray(sd["decoder.pointer.project_out.weight"], np.float64).T, None, rnd)
    out["gctx"] = (emb.mean(1) @ np.asarray(sd["decoder.project_fixed_context.weight"], np.float64).T
                   if use_graph_context else None)
    return out


def rel_err(a, b):
    """Relative Frobenius error |a - b| / |b|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
