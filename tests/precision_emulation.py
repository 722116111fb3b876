"""The 16-bit encoder contract ("16-bit encoder") restated in float64 numpy, rounding to T at exactly the
contract's points, for comparison with eamrl_encoder_fused16.  With `rnd=None` nothing is rounded and the emulation is
the fp32 encoder + cache of the oracle in float64.

`encode` / `precompute` take a policy's state dict.  `run_contract` below is the same contract stage by stage on plain
weight arrays (the arguments of ops.encoder_fused16), with the switches the contract tests need: the kernel's d_expf cut-off
and fp32 division mirrored, fp32 accumulation instead of float64, an exactness trace, and one-line mutants."""
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


# ---- the contract stage by stage, on the arguments of ops.encoder_fused16 --------------------------------------------------

E, H, FF = 128, 8, 512
SLOTS = ("K", "V", "L", "Pa", "Pb")

# one-line variants of the contract that a correct test must tell from the contract itself
MUTANTS = ("unmasked", "mask_m1", "mask_p1", "pad_tile", "heads_swapped", "tiles_swapped", "w1_chunks", "lp_unrounded_l",
           "lp_from_k", "w_unrounded", "z_unrounded", "hidden_unrounded", "input_unrounded", "bias_rounded",
           "residual_rounded", "o_unrounded")


def padded_rows(M):
    """Rows of the kernel variant that holds M nodes: 16 * RTT."""
    return 32 if M <= 32 else 64 if M <= 64 else 112


def quantum(*xs):
    """The largest power of two of which every element of every array is a multiple."""
    xs = [np.asarray(x, np.float64) for x in xs]
    for p in range(-40, 80):
        if all(np.array_equal(np.ldexp(x, p), np.rint(np.ldexp(x, p))) for x in xs):
            return 2.0 ** -p
    raise ValueError("no power-of-two quantum above 2^-80")


def d_expf(x):
    """dmath.hpp's d_expf for x <= 0 in fp32, step by step (each fma as the fp32 rounding of the float64 result): exactly 1 at
    0 and exactly 0 below -87."""
    f32, f64 = np.float32, np.float64
    x = np.asarray(x, f32)
    fma = lambda a, b, c: (a.astype(f64) * f64(b) + np.asarray(c, f64)).astype(f32)
    xc = np.where(x >= -87, x, f32(0))
    n = np.rint(xc * f32(1.44269504088896341))
    r = fma(n, f32(-0.693359375), xc)
    r = fma(n, f32(2.12194440e-4), r)
    p = np.full_like(r, f32(1.9875691500e-4))
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = fma(p, r, f32(c))
    y = fma(p, r * r, r) + f32(1)
    return np.where(x >= -87, np.ldexp(y, n.astype(np.int32)), f32(0)).astype(f32)


class Trace:
    """What the exactness certificate of an integer-grid case needs to know about one run."""

    def __init__(self):
        self.gemm = {}              # name -> max over outputs of (sum |a b| + |bias|) / quantum of the terms
        self.rounded = set()        # rounding points that changed a value
        self.not_fp32 = set()       # fp32 storage points whose float64 value is not an fp32 number
        self.score_gap = True       # every score minus its row maximum is 0 or below -87
        self.max_tie = 0            # largest number of keys sharing the row maximum
        self.adversary = None       # share of (query, head) pairs in which an unmasked padded key would hold the maximum


class _Run:
    def __init__(self, rnd, acc, div32, mutant, trace):
        if mutant is not None and mutant not in MUTANTS:
            raise ValueError(f"unknown mutant {mutant!r}")
        self.rnd, self.acc, self.div32, self.mut, self.trace = rnd or _id, acc, div32, mutant, trace

    def f(self, x, where=None):
        """An fp32 value of the kernel (float64 here unless acc is float32)."""
        y = np.asarray(x, self.acc)
        if self.trace is not None and where and not np.array_equal(y, np.asarray(y, np.float32)):
            self.trace.not_fp32.add(where)
        return y

    def r(self, x, where):
        y = self.rnd(x)
        if self.trace is not None and not np.array_equal(y, np.asarray(x, np.float64)):
            self.trace.rounded.add(where)
        return y.astype(self.acc)

    def mm(self, a, bT, bias, where):
        """a [.., n, k] x bT [.., k, c] with the fp32 bias as the accumulator's initial value."""
        if bias is not None:
            bias = self.r(bias, "bias") if self.mut == "bias_rounded" else self.f(bias)
        if self.acc is np.float32:      # one k-ordered fp32 chain per output: the same numbers on every host, whatever its BLAS
            y = np.zeros(a.shape[:-1] + bT.shape[-1:], np.float32) + (0.0 if bias is None else bias)
            for k in range(a.shape[-1]):
                y += a[..., :, k, None] * bT[..., k, None, :]
        else:
            y = np.matmul(a, bT)
            if bias is not None:
                y = y + bias
        if self.trace is not None:
            s = np.matmul(np.abs(a), np.abs(bT))
            q = quantum(a) * quantum(bT)
            if bias is not None:
                s, q = s + np.abs(bias), min(q, quantum(bias))
            self.trace.gemm[where] = max(self.trace.gemm.get(where, 0.0), float(s.max() / q))
        return self.f(y, where)

    def linear(self, x, W, b, where):
        return self.mm(x, self.r(W, "weights").T, b, where)

    def operand(self, h):
        return self.f(h) if self.mut == "input_unrounded" else self.r(h, "h")

    def attention(self, qkv, bqkv):
        B, M, _ = qkv.shape
        D = E // H
        heads = lambda x: x.reshape(B, -1, H, D).transpose(0, 2, 1, 3)
        q = heads(self.r(qkv[..., :E] * 0.25, "q"))
        k = heads(self.r(qkv[..., E:2 * E], "k"))
        v = heads(self.r(qkv[..., 2 * E:], "v"))
        # rows M .. of the kernel's tiles are h = 0 (first layer): k = bk, v = bv there, masked by the contract
        rows = padded_rows(M)
        kpad = np.broadcast_to(self.r(bqkv[E:2 * E], "k").reshape(1, H, 1, D), (B, H, 1, D))
        vpad = np.broadcast_to(self.r(bqkv[2 * E:], "v").reshape(1, H, 1, D), (B, H, 1, D))
        if self.trace is not None and rows > M:
            top = np.matmul(q, k.transpose(0, 1, 3, 2)).max(-1)
            self.trace.adversary = float((np.matmul(q, kpad.transpose(0, 1, 3, 2))[..., 0] > top).mean())
        extra, vextra = 0, None
        if self.mut == "unmasked":
            extra, vextra = rows - M, 0.0 * vpad
        elif self.mut == "mask_p1":
            extra, vextra = min(1, rows - M), 0.0 * vpad
        elif self.mut == "pad_tile":
            extra, vextra = rows - 16 * ((M + 15) // 16), vpad
        if extra:
            k = np.concatenate([k, np.repeat(kpad, extra, 2)], 2)
            v = np.concatenate([v, np.repeat(vextra, extra, 2)], 2)
        s = self.mm(q, k.transpose(0, 1, 3, 2), None, "scores")
        if self.mut == "mask_m1" and M > 1:
            s[..., M - 1] = -np.inf
        e = self.f(s - s.max(-1, keepdims=True))
        if self.trace is not None:
            self.trace.score_gap &= bool(np.all((e == 0) | (e < -87)))
            self.trace.max_tie = max(self.trace.max_tie, int((e == 0).sum(-1).max()))
        w = d_expf(e) if self.acc is np.float32 else np.where(e >= -87, np.exp(np.maximum(e, -87.0)), 0.0)
        wt = self.r(w, "w")
        z = (w if self.mut == "z_unrounded" else wt).sum(-1, keepdims=True)
        o = self.mm(w if self.mut == "w_unrounded" else wt, v, None, "value product")
        if self.div32:      # the kernel's correctly rounded fp32 division
            o = (o.astype(np.float32) / z.astype(np.float32)).astype(self.acc)
        else:
            o = self.f(o / z)
        return o.transpose(0, 2, 1, 3).reshape(B, M, E)

    def norm(self, Ly, p, h, norm, eps):
        g, b = self.f(Ly[p + "_gamma"]), self.f(Ly[p + "_beta"])
        if norm == "batch":
            sc = self.f(g / np.sqrt(self.f(self.f(Ly[p + "_var"]) + self.acc(eps))), "norm scale")
            sh = self.f(b - self.f(self.f(Ly[p + "_mean"]) * sc, "norm shift"), "norm shift")
            h = self.f(h * sc + sh, "norm")
        else:
            mean = h.mean(1, keepdims=True, dtype=self.acc)
            var = ((h - mean) ** 2).mean(1, keepdims=True, dtype=self.acc)
            h = self.f((h - mean) * (1.0 / np.sqrt(var + self.acc(eps))) * g + b)
        return self.r(h, "residual") if self.mut == "residual_rounded" else h

    def layer(self, Ly, h, norm, eps):
        qkv = self.linear(self.operand(h), Ly["Wqkv"], Ly["bqkv"], "qkv")
        att = self.attention(qkv, Ly["bqkv"])
        att = self.f(att) if self.mut == "o_unrounded" else self.r(att, "o")
        if self.mut == "heads_swapped":
            att = np.concatenate([att[..., :16], att[..., 80:96], att[..., 32:80], att[..., 16:32], att[..., 96:]], -1)
        h = self.norm(Ly, "n1", self.f(h + self.linear(att, Ly["Wo"], Ly["bo"], "out_proj"), "residual"), norm, eps)
        W1 = self.r(Ly["W1"], "weights")
        if self.mut == "tiles_swapped":
            W1 = np.concatenate([W1[16:32], W1[:16], W1[32:]], 0)
        hid = np.maximum(self.mm(self.operand(h), W1.T, Ly["b1"], "ffn1"), 0.0)
        hid = self.f(hid) if self.mut == "hidden_unrounded" else self.r(hid, "hidden")
        if self.mut == "w1_chunks":
            hid = np.concatenate([hid[..., :128], hid[..., 256:384], hid[..., 128:256], hid[..., 384:]], -1)
        return self.norm(Ly, "n2", self.f(h + self.linear(hid, Ly["W2"], Ly["b2"], "ffn2"), "residual"), norm, eps)

    def cache(self, h, c):
        x = self.operand(h)
        out = {n: self.linear(x, c["Wc"][i * E:(i + 1) * E], None, n) for i, n in enumerate(SLOTS[:c["nproj"]])}
        L = out["K"] if self.mut == "lp_from_k" else out["L"]
        out["Lp"] = self.linear(self.f(L) if self.mut == "lp_unrounded_l" else self.r(L, "L"), c["WoutT"], None, "Lp")
        if c.get("Wg") is not None:     # fp32 path: the mean over the nodes, then the one-row Linear, nothing rounded
            mean = self.f(self.f(h.sum(1, dtype=self.acc), "gctx") / self.acc(h.shape[1]), "gctx")
            out["gctx"] = self.mm(mean, self.f(c["Wg"]).T, None, "gctx")
        return out


def run_contract(layers, h, rnd=None, norm="batch", eps=1e-5, cache=None, acc=np.float64, div32=False, mutant=None,
                 trace=None):
    """h [B, M, E] through `layers` (dicts of the fields of struct eamrl_encoder_layer, unpacked fp32 weights) and, with
    cache = dict(Wc [nproj E, E], WoutT [E, E], nproj[, Wg [E, E]]), the decoder cache.  Returns {"h", "K", "V", "L", "Pa"
    (, "Pb"), "Lp" (, "gctx")} as float64.

    acc=np.float32: every product, sum and elementwise step in fp32 with the same rounding points (the yardstick of what
    fp32 accumulation alone moves).  div32: `o / Z` as the kernel's correctly rounded fp32 division (differs from float64
    only at rounding ties).  mutant: one of MUTANTS.  trace: a Trace to fill."""
    run = _Run(rnd, acc, div32, mutant, trace)
    h = run.f(h)
    for Ly in layers:
        h = run.layer(Ly, h, norm, eps)
    out = {"h": h}
    if cache is not None:
        out.update(run.cache(h, cache))
    return {n: np.asarray(v, np.float64) for n, v in out.items()}


def row_err(a, b):
    """Per-row relative error |a_row - b_row|_2 / |b_row|_2 over the last axis (0 where both rows are zero)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d, n = np.linalg.norm(a - b, axis=-1), np.linalg.norm(b, axis=-1)
    return np.where(d == 0, 0.0, d / np.maximum(n, 1e-30))
