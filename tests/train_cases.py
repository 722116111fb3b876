"""The cases of the training-graph kernel tests (tests/test_host_train_ref.py on the CPU, tests/test_gpu_train_kernels.py on the
GPU): named shapes that reach every branch of the launch functions, operands from a seeded generator, the float64 / float32 runs
of the restatements (tests/train_ref.py), computed once per case and shared, and the bound of every compared output.

Families (`fam`) and the kernels behind them:
  linear    ops.linear_wgrad             k_linear_wgrad, k_wgrad_reduce            (csrc/train_gemm.hip)
  small     ops.small_linear_wgrad       k_small_wgrad_partial / _final            (csrc/train_norm.hip)
  instnorm  ops.instance_norm_forward / _backward   k_instnorm_train_fwd / _bwd    (csrc/encoder.hip)
  bn        ops.batchnorm_backward       k_bn_bwd_partial / _final / _dx           (csrc/train_norm.hip)
  attn      ops.mha_encoder / ops.mha_encoder_backward up to 112 nodes: k_mha_encoder_bwd (csrc/reeval.hip)

Data kinds:
  normal    unit-scale randn
  offset    the norms: x = 1000 + randn (a one-pass variance loses every digit).  The two weight gradients: x = 1000 + randn and
            dy with alternating sign over the rows, so the true sum nearly cancels
  const     the norms: three channels constant over the nodes / rows, so the variance is exactly zero: rstd = 1 / sqrt(eps) and
            y == beta there.  The constants (0.5, -3, 1000) are chosen so that every partial sum k c, k <= N, is a float32 number:
            the mean is then c in ANY summation order.  (With a constant whose partial sums round, mean != c is legitimate
            float32 rounding, and y - beta is that residue times rstd = 316.)
  tiny      the norms: x = 1e-20 randn: (x - mean)^2 underflows, the variance vanishes beside eps
(offset and const have no meaning for the attention; const and tiny none for the weight gradients, which keep no statistic.)

Bounds (none comes from the kernels).  The error of an output against the float64 run is the max-abs difference for the values
(y, mean, rstd) and the norm of the difference for the gradients.  It may be at most MARGIN (4, as tests/reeval_cases.py and
tests/test_gpu_filter.py) times RATIO[family, output, kind] (1 unless recorded otherwise below) times the larger of
  - the same error figure of the restatement's float32 run, and
  - the floor U = 2^-24 times the output's own magnitude: the largest per-entry sum of |terms| for the sums (dW, db, dgamma,
    dbeta, mean), the largest |value| otherwise.  The floor is there because the float32 run is exact or nearly so at rows = 1,
    N = 1 and in the const channels.
An output that is exactly zero in float64 gets the bound 0 through the same rule (its magnitude is 0): it must be exactly zero.
These are, with the reason the kernels' formulas make them exact:
  instnorm N = 1    dx: dy - mean(dy) = g - g / 1 = 0 and xhat = (x - x / 1) rstd = 0;  dgamma: every term is dy * 0
  bn rows = 1       dx, dgamma: the same (the kernel is handed mean = x, var = 0)
No output that is zero in float64 is left inexact by a kernel's formula, so no such output needs the floor of its neighbours.
"""
import functools

import torch

import train_ref as tr
from reeval_cases import MARGIN        # 4.0: over a float32-vs-float64 difference

U = 2.0 ** -24
EPS = float(torch.tensor(1e-5, dtype=torch.float32))       # the float32 the kernels receive
H, E_ATT = 8, 128
VALUES = ("y", "mean", "rstd")
OUTPUTS = dict(linear=("dW", "db"), small=("dW", "db"), instnorm=("y", "mean", "rstd", "dx", "dgamma", "dbeta"),
               bn=("dx", "dgamma", "dbeta"), attn=("y", "dqkv"))
PLANTS = ("row_dropped", "last_chunk_dropped", "one_pass_variance")
CONST_VALUES = (0.5, -3.0, 1000.0)
# Kernel error allowed over the scale (the larger of the float32 restatement's error and the floor), per (family, output, data
# kind): MARGIN times RATIO, 1 unless a measured ratio is recorded here with its case and the arithmetic that explains it (as
# reeval_cases.RATIO).
# linear db on the offset data: k_linear_wgrad feeds the MFMA two rows at a time, and lane l of a wavefront adds the dy of the rows
# of parity l >> 5 to its own bias sum (bs0 += a0); the two parities meet in one shuffle at the end.  With dy = +-(1 + 0.1 randn)
# alternating over the rows, one lane sums only the +1 rows and the other only the -1 rows: each partial sum grows to rows / 2 and
# every add rounds at that size (half an ulp of 32: 1.9e-6, about 33 adds of it at 66 rows), where the restatement's sum in row
# order stays near 1 throughout.  Per entry the kernel's error is 2.6e-6, inside U sum |terms| = 4.1e-6; the compared figure is
# the norm over the 128 entries, 11 times that.  Measured on the MI355X: 7.21 times the scale at lin_r66_128x128_offset (2.93e-5
# against the floor 4.06e-6; the restatement: 1.5e-6), 6.09 at lin_r193_128x128_offset -- rounding in another order, not a
# defect.  dW of the same cases stays at 1.0 (an MFMA adds an even and an odd row into one accumulator), and db on the normal
# data at 1.71.
RATIO = {("linear", "db", "offset"): 7.21}


def const_channels(E):
    return (0, E // 2, E - 1)


def linear_chunks(rows, out_dim, in_dim):
    """(chunks, rows per chunk) of k_linear_wgrad as the issue states them: min(ceil(512 / blocks), ceil(rows / 64)) chunks of
    ceil(rows / chunks) rows rounded up to 16."""
    blocks = (out_dim // 128) * (in_dim // 128)
    nch = max(1, min(-(-512 // blocks), -(-rows // 64)))
    return nch, -(-(-(-rows // nch)) // 16) * 16


def instnorm_lds(N, E):
    """(bytes, regime) of k_instnorm_train_fwd: the [N][E] tile and two [E] rows in LDS."""
    b = (N * E + 2 * E) * 4
    return b, ("lds" if b <= 64 * 1024 else "lds_raised" if b <= 96 * 1024 else "global")


def _case(name, fam, **kw):
    c = dict(name=name, fam=fam, kind="normal", strided=None, no_aux=False)
    c.update(kw)
    return c


def _build():
    cs = []

    # ---- ops.linear_wgrad: (rows, out, in, declared chunk count) -------------------------------------------------------------
    def lin(rows, o, i, nch, **kw):
        tag = "".join(f"_{v}" for v in (kw.get("kind", "normal"), kw.get("strided"), "noaux" if kw.get("no_aux") else None)
                      if v not in (None, "normal"))
        return _case(f"lin_r{rows}_{o}x{i}{tag}", "linear", rows=rows, out=o, inp=i, nch=nch, **kw)

    # one chunk: 1 / 15 rows in a slab, a full slab, a 1-row second slab, a 15-row and a full fourth slab
    cs += [lin(r, 128, 128, 1) for r in (1, 15, 16, 17, 63, 64)]
    cs += [lin(65, 128, 128, 2, no_aux=True),      # two chunks of 48 rows, the second holds 17; need_bias=False beside it
           lin(193, 128, 128, 4),                  # chunks of 64 rows, the last chunk is 1 row
           lin(769, 128, 128, 13),                 # 13 chunks: thread group 0 alone takes one trip of k_wgrad_reduce's unrolled loop
           lin(1025, 128, 128, 17)]                # 17 chunks: the unrolled trip for every group, group 0 a tail of one
    # grid x > 1 and y > 1: the bias sums come from blockIdx.y == 0 only
    for o, i in ((384, 128), (128, 512), (512, 512)):
        cs += [lin(65, o, i, 2), lin(777, o, i, 13)]
    # capped chunking: nch = 512 / blocks, rows per chunk rounded up to 16, trailing chunks start beyond `rows` (nslab <= 0)
    cs += [lin(2049, 512, 512, 32, no_aux=True),   # 32 chunks of 80 rows: chunk 25 holds 49, chunks 26 .. 31 are empty
           lin(32769, 128, 128, 512)]              # 512 chunks of 80 rows: chunk 409 holds 49, chunks 410 .. 511 are empty
    # column slices of wider tensors: ldy, ldx are not the dims
    cs += [lin(193, 128, 128, 4, strided="both"), lin(777, 384, 128, 13, strided="both")]
    cs += [lin(66, 128, 128, 2, kind="offset"), lin(193, 128, 128, 4, kind="offset")]

    # ---- ops.small_linear_wgrad: chunks of 256 rows ---------------------------------------------------------------------------
    def sm(rows, K, o, **kw):
        tag = "".join(f"_{v}" for v in (kw.get("kind", "normal"), kw.get("strided"), "noaux" if kw.get("no_aux") else None)
                      if v not in (None, "normal"))
        return _case(f"sm_r{rows}_K{K}_o{o}{tag}", "small", rows=rows, K=K, out=o, **kw)

    cs += [sm(257, K, 128) for K in range(1, 9)]                       # every K; two chunks, the second of 1 row
    cs += [sm(r, 2, 128) for r in (1, 255, 256, 2000)]                 # one row, both sides of the chunk, 8 chunks (the last of 208)
    cs += [sm(257, 3, 64),                                             # one wavefront
           sm(257, 3, 100), sm(1, 5, 100),                             # 128 threads, the guard o < out_dim
           sm(257, 7, 300), sm(2000, 8, 300)]                          # 256 threads, the strided o loop (second trip partial)
    cs += [sm(2000, 6, 128, strided="x"), sm(257, 4, 100, strided="dy"), sm(257, 2, 128, no_aux=True),
           sm(257, 3, 128, kind="offset")]

    # ---- ops.instance_norm_forward / _backward ----------------------------------------------------------------------------------
    def inn(B, N, E, **kw):
        tag = "".join(f"_{v}" for v in (kw.get("kind", "normal"), "noaux" if kw.get("no_aux") else None) if v not in (None, "normal"))
        return _case(f"in_B{B}_N{N}_E{E}{tag}", "instnorm", B=B, N=N, E=E, **kw)

    cs += [inn(3, N, 128) for N in (1, 2, 3, 4, 5)]                    # fewer rows than the backward's four row groups (N = 5: one
    cs += [inn(1, 1, 128)]                                             # group has two)
    cs += [inn(3, 126, 128),                                           # 65,536 bytes: the last size without the raised attribute
           inn(3, 127, 128), inn(1, 127, 128),                         # 66,048 bytes: the first with it
           inn(3, 190, 128),                                           # 98,304 bytes: the last size in LDS
           inn(3, 191, 128),                                           # 98,816 bytes: the global-memory walk (in_lds == 0)
           inn(3, 300, 128)]
    cs += [inn(3, 20, 6),                                              # a tiny E (scalar staging, one partial wavefront per group)
           inn(3, 20, 64),
           inn(3, 20, 130),                                            # scalar staging (E % 4 != 0); two backward passes, 2 channels
           inn(3, 20, 200, no_aux=True),                               # two backward passes, the second partial (72 of 128)
           inn(3, 20, 300)]                                            # the forward's e += 256 loop; three backward passes
    cs += [inn(2, 187, 130),                                           # 98,280 bytes: scalar staging with the raised attribute
           inn(2, 188, 130)]                                           # 98,800 bytes: E % 4 != 0 on the global-memory walk
    cs += [inn(1, 20, 128), inn(3, 20, 128, no_aux=True),
           inn(600, 20, 128)]                                          # the atomics of 600 workgroups on dgamma / dbeta
    cs += [inn(3, 20, 128, kind=k) for k in ("offset", "const", "tiny")]
    cs += [inn(3, 3, 128, kind="offset"), inn(3, 20, 130, kind="const"), inn(3, 20, 300, kind="offset")]

    # ---- ops.batchnorm_backward: chunks of 128 rows ---------------------------------------------------------------------------
    def bn(rows, E, **kw):
        tag = "".join(f"_{v}" for v in (kw.get("kind", "normal"), "noaux" if kw.get("no_aux") else None) if v not in (None, "normal"))
        return _case(f"bn_r{rows}_E{E}{tag}", "bn", rows=rows, E=E, **kw)

    cs += [bn(1, 128),                                                 # var = 0: dx and dgamma exactly 0
           bn(2, 128), bn(127, 128), bn(128, 128), bn(129, 128, no_aux=True), bn(5000, 128),      # chunk edges; 40 chunks
           bn(32769, 128)]                                             # 1,048,608 float4: the grid-stride second trip of k_bn_bwd_dx
    cs += [bn(129, 4), bn(129, 64), bn(129, 200, no_aux=True),
           bn(129, 1028), bn(300, 2048)]                               # more than 1024 channels: the channel loop at 1024 threads
    cs += [bn(129, 128, kind=k) for k in ("offset", "const", "tiny")]

    # ---- ops.mha_encoder_backward up to 112 nodes: key tiles of 16, kernels for <= 32 / <= 64 / <= 112 keys --------------------
    def at(N, amp, **kw):
        return _case(f"at_N{N}_a{amp}" + ("_tie" if kw.get("tie") else ""), "attn", B=2, N=N, amp=amp, **kw)

    cs += [at(N, 1.5) for N in (1, 2, 15, 16, 17, 32, 33, 63, 64, 65, 111, 112)]
    cs += [at(N, 6) for N in (17, 33, 64, 112)]                        # a peaked softmax
    cs += [at(33, 1.5, tie=True)]                                      # two bit-identical nodes (0 and N - 2)
    return {c["name"]: c for c in cs}


CASES = _build()
NAMES = list(CASES)


def outputs(c):
    """The outputs compared in case c."""
    return list(OUTPUTS[c["fam"]])


def operands(name):
    """-> dict of the case's operands (float32 CPU tensors)."""
    c = CASES[name]
    g = torch.Generator().manual_seed(2000 + NAMES.index(name))
    fam, kind = c["fam"], c["kind"]

    def randn(*shape):
        return torch.randn(*shape, generator=g)

    if fam in ("linear", "small"):
        rows, o = c["rows"], c["out"]
        i = c["inp"] if fam == "linear" else c["K"]
        if kind == "offset":
            sign = 1.0 - 2.0 * (torch.arange(rows) % 2).float()
            return dict(dy=sign[:, None] * (1.0 + 0.1 * randn(rows, o)), x=1000.0 + randn(rows, i))
        return dict(dy=randn(rows, o), x=randn(rows, i) if fam == "linear" else torch.rand(rows, i, generator=g))
    if fam in ("instnorm", "bn"):
        E = c["E"]
        lead = (c["B"], c["N"]) if fam == "instnorm" else (c["rows"],)
        x = {"normal": lambda: randn(*lead, E) * 2 + 0.5, "const": lambda: randn(*lead, E) * 2 + 0.5,
             "offset": lambda: 1000.0 + randn(*lead, E), "tiny": lambda: 1e-20 * randn(*lead, E)}[kind]()
        if kind == "const":
            for ch, v in zip(const_channels(E), CONST_VALUES):
                x[..., ch] = v
        return dict(x=x, gamma=torch.rand(E, generator=g) + 0.5, beta=randn(E), dy=randn(*lead, E))
    qkv = randn(c["B"], c["N"], 3 * E_ATT) * c["amp"]
    if c.get("tie"):
        qkv[:, c["N"] - 2] = qkv[:, 0]
    return dict(qkv=qkv, dout=randn(c["B"], c["N"], E_ATT))


def run_restatement(c, op, dtype, **kw):
    """-> dict of the restatement's outputs for case c in `dtype`."""
    fam = c["fam"]
    if fam == "linear":
        return dict(zip(("dW", "db"), tr.linear_wgrad(op["dy"], op["x"], dtype)))
    if fam == "small":
        return dict(zip(("dW", "db"), tr.small_linear_wgrad(op["dy"], op["x"], dtype)))
    if fam == "instnorm":
        return dict(zip(OUTPUTS[fam], tr.instance_norm(op["x"], op["gamma"], op["beta"], EPS, op["dy"], dtype, **kw)))
    if fam == "bn":
        return dict(zip(("mean", "var", "dx", "dgamma", "dbeta"), tr.batchnorm_backward(op["x"], op["dy"], op["gamma"], EPS, dtype, **kw)))
    return dict(zip(("y", "dqkv"), tr.attention_backward(op["qkv"], op["dout"], H, dtype, **kw)))


def _scales(c, op, r64):
    """The magnitude of every output (float64): per-entry sums of |terms| for the sums, the largest |value| otherwise."""
    fam = c["fam"]
    s = {k: float(r64[k].abs().max()) for k in outputs(c)}
    if fam in ("linear", "small"):
        dy, x = op["dy"].double().abs(), op["x"].double().abs()
        s.update(dW=float((dy.t() @ x).max()), db=float(dy.sum(0).max()))
    elif fam == "instnorm":
        x, dy = op["x"].double(), op["dy"].double()
        xhat = (x - r64["mean"][:, None]) * r64["rstd"][:, None]
        s.update(mean=float(x.abs().mean(1).max()), dgamma=float((dy * xhat).abs().sum((0, 1)).max()),
                 dbeta=float(dy.abs().sum((0, 1)).max()))
    elif fam == "bn":
        x, dy = op["x"].double(), op["dy"].double()
        xhat = (x - r64["mean"]) / torch.sqrt(r64["var"] + EPS)
        s.update(dgamma=float((dy * xhat).abs().sum(0).max()), dbeta=float(dy.abs().sum(0).max()))
    return s


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (op, r64, r32): the operands, the float64 and the float32 run of the restatement; r64["_scale"] holds the outputs'
    magnitudes.  A batch-norm case hands the float32 run (as the GPU test hands the kernel) the float64 mean and biased variance
    rounded to float32: op["mean"], op["var"].  Computed once; nothing may modify it."""
    c = CASES[name]
    op = operands(name)
    r64 = run_restatement(c, op, torch.float64)
    if c["fam"] == "bn":
        op["mean"], op["var"] = r64["mean"].float(), r64["var"].float()
        r32 = run_restatement(c, op, torch.float32, stats=(op["mean"], op["var"]))
    else:
        r32 = run_restatement(c, op, torch.float32)
    r64["_scale"] = _scales(c, op, r64)
    return op, r64, r32


def error(name, got, r64):
    """The error figure of output `name`: max-abs for a value, the norm of the difference for a gradient tensor."""
    d = got.double() - r64[name]
    return float(d.abs().max()) if name in VALUES else float(d.norm())


def bound(c, name, r64, r32):
    """-> (kind, bound) of output `name` of case c; kind: "maxabs" or "norm"."""
    scale = max(error(name, r32[name], r64), U * r64["_scale"][name])
    return ("maxabs" if name in VALUES else "norm"), MARGIN * RATIO.get((c["fam"], name, c["kind"]), 1.0) * scale


def misses(c, got, r64, r32, names=None):
    """[(output, kind, figure, bound)] of the compared outputs of `got` that lie beyond their bound."""
    bad = []
    for name in names or outputs(c):
        kind, bd = bound(c, name, r64, r32)
        fig = error(name, got[name], r64)
        if not fig <= bd:
            bad.append((name, kind, fig, bd))
    return bad


def last_chunk_start(c):
    """The first row of the last non-empty chunk of the case's contraction (of the last 16-row slab where there is one chunk)."""
    fam = c["fam"]
    if fam == "linear":
        nch, rpc = linear_chunks(c["rows"], c["out"], c["inp"])
        return (c["rows"] - 1) // (rpc if nch > 1 else 16) * (rpc if nch > 1 else 16)
    if fam == "small":
        return (c["rows"] - 1) // 256 * 256
    if fam == "bn":
        return (c["rows"] - 1) // 128 * 128
    return (c["N"] - 1) // 16 * 16         # attn: the last key tile


def planted(name, which):
    """-> the float64 outputs of case `name` with a deliberate error, or None where the case has no room for it:
      row_dropped          the last row (node, key) left out of the contraction; none where the contraction has one term and the
                           result without it is not defined (N = 1, rows = 1 of the norms, one key)
      last_chunk_dropped   the last chunk (slab, key tile) left out; the instance norm: the backward's last row group n = 3 (mod 4)
      one_pass_variance    the norms on `offset` data: the variance as mean(x^2) - mean(x)^2 in float32"""
    c = CASES[name]
    op, r64, _ = reference(name)
    fam = c["fam"]
    assert which in PLANTS
    if which == "one_pass_variance":
        if c["kind"] != "offset" or fam not in ("instnorm", "bn"):
            return None
        if fam == "instnorm":
            return {k: v.double() for k, v in run_restatement(c, op, torch.float32, one_pass=True).items()}
        x = op["x"]
        var = ((x * x).mean(0) - x.mean(0) ** 2).clamp_min(0)
        return run_restatement(c, op, torch.float64, stats=(r64["mean"], var))
    n = c["N"] if fam in ("instnorm", "attn") else c["rows"]
    if fam == "instnorm":
        keep = torch.ones(n, dtype=torch.bool)
        if which == "row_dropped":
            keep[-1] = False
        else:
            keep[3::4] = False
        if n < 2 or keep.all():
            return None
        x, dy, gamma = op["x"].double(), op["dy"].double(), op["gamma"].double()
        xhat = (x - r64["mean"][:, None]) * r64["rstd"][:, None]
        w = keep.double()[None, :, None]
        m1, m2 = (dy * w).sum(1) / n, (dy * xhat * w).sum(1) / n
        dx = (gamma * r64["rstd"])[:, None] * (dy - m1[:, None] - xhat * m2[:, None])
        return dict(y=r64["y"], mean=r64["mean"], rstd=r64["rstd"], dx=dx, dgamma=(dy * xhat * w).sum((0, 1)), dbeta=(dy * w).sum((0, 1)))
    start = n - 1 if which == "row_dropped" else last_chunk_start(c)
    if fam == "attn":
        return None if start < 1 else run_restatement(c, op, torch.float64, keys=start)
    if fam == "bn":
        if n < 2:
            return None
        x, dy, gamma = op["x"].double(), op["dy"].double(), op["gamma"].double()
        rstd = 1.0 / torch.sqrt(r64["var"] + EPS)
        xhat = (x - r64["mean"]) * rstd
        dbeta, dgamma = dy[:start].sum(0), (dy * xhat)[:start].sum(0)
        return dict(dx=gamma * rstd * (dy - dbeta / n - xhat * (dgamma / n)), dgamma=dgamma, dbeta=dbeta)
    return run_restatement(c, dict(dy=op["dy"][:start], x=op["x"][:start]), torch.float64)
