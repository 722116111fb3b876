"""The cases of the large-graph encoder attention tests (tests/test_host_attention_large.py on the CPU,
tests/test_gpu_attention_large.py on the GPU): named sizes on every edge of the three kernels, operands from a seeded generator,
the float64 / float32 runs of the restatement (tests/train_ref.py: attention_backward), computed once per case and shared, the
bound of every compared output, and the planted errors the bound must reject.  The protocol is that of tests/train_cases.py.

The kernels:
  k_mha_encoder_mfma        (csrc/encoder_attn_mfma.hip)      forward, 128 .. 1200 nodes: NT = ceil(N / 16) key tiles staged in
                            NT x 2048 bytes of LDS (the raised attribute above 64 KiB: N >= 513; the limit 150 KiB: N = 1200), the
                            scores walked four tiles at a time (the tiles beyond the last one clamped: NT % 4)
  k_mha_encoder_tiled       (csrc/encoder.hip)                the VALU forward, keys in LDS tiles of 128: above 1200 nodes, and
                            under debug key 15
  k_mha_encoder_bwd_mfma<U> (csrc/encoder_attn_bwd_mfma.hip)  backward, 113 .. 1024 nodes: wave w of 8 owns the key tiles
                            w, w + 8, ...: U = ceil(NT / 8) of them, one instantiation per U; NT x 2048 + 29,696 bytes of LDS

Data kinds (qkv [B, N, 384] packed q | k | v of 8 heads, dout [B, N, 128] = randn):
  normal     qkv = 1.5 randn
  peaked     qkv = 6 randn: scores of some hundreds, the largest weight above 0.999
  twin       normal, node N - 2 a bit copy of node 0 (at 257 nodes the two sit in different waves' tiles)
  dominant   qkv = 0.1 randn, plus in every (instance, head) a unit direction u: sqrt(48) u added to every query and to ONE key `dom`,
             which then scores 48 / sqrt(16) = 12 above the rest in every row: its weight is 0.98 .. 0.9999, and the partials of
             the waves that do not hold it are rescaled by about exp(-12).  (Not more: at a gap of 60 the float64 dq and dk are
             about 1e-23 and the comparison is empty.)
  zero_rows  normal, dout rows 0, 17 and N - 1 exactly zero: dq of those rows is exactly zero (dP = 0, X = 0, Delta = 0, dS = P * 0)

Outputs, each compared on its own: y, and the three column blocks dq | dk | dv of dqkv.  The forward-only cases (above the
backward's 1024 nodes) compare y alone.

Bounds (none comes from the kernels).  The error of an output against the float64 run is the max-abs difference for y and the
norm of the difference for dq, dk, dv.  It may be at most MARGIN (4, tests/reeval_cases.py) times RATIO[output, kind] (1 unless
recorded below) times the larger of
  - the same error figure of the restatement's float32 run, and
  - the floor 2^-24 max |output| (float64).
"""
import functools
import math

import torch

import train_ref as tr
from reeval_cases import MARGIN        # 4.0: over a float32-vs-float64 difference

U = 2.0 ** -24
H, E = 8, 128
D = E // H
OUTPUTS = ("y", "dq", "dk", "dv")
KINDS = ("normal", "peaked", "twin", "dominant", "zero_rows")
AMP = dict(normal=1.5, peaked=6.0, twin=1.5, dominant=0.1, zero_rows=1.5)
DOMINANT_GAP = 12.0
ZERO_ROWS = (0, 17, -1)
PLANTS = ("last_key_dropped", "last_key_tile_dropped", "wave7_key_tiles_dropped", "last_query_tile_skipped")
# Kernel error allowed over the scale, per (output, data kind): MARGIN times RATIO, 1 unless a measured ratio is recorded here with
# its case and the arithmetic that explains it (as train_cases.RATIO and reeval_cases.RATIO).  There is none.
RATIO = {}

# the sizes, by the edge each sits on
BWD_U_STEPS = (128, 129, 256, 257, 384, 385, 512, 513, 640, 641, 768, 769, 896, 897)       # both sides of every U step
BWD_NORMAL = (113, 127) + BWD_U_STEPS + (272, 273, 1023, 1024)
BWD_PEAKED = (129, 641, 1024)
BWD_DOMINANT = ((113, 112), (273, 272), (641, 640), (1024, 1023), (1024, 0), (897, 115))    # (N, the dominant key)
FWD_ONLY = (1185, 1200, 1201, 1281)
# the forward against the oracle, bit for bit (tests/test_gpu_attention_large.py)
ORACLE_SIZES = (128, 129, 144, 145, 160, 161, 176, 177, 192, 193, 511, 512, 513, 1023, 1024, 1185, 1200, 1201, 1281)
ORACLE_KINDS = ("normal", "peaked", "twin", "dominant")


# ---- the launch rules, restated from the formulas of the two .hip files ---------------------------------------------------------
def key_tiles(N):
    """NT: the 16-key tiles of both MFMA kernels."""
    return (N + 15) // 16


def bwd_tiles_per_wave(N):
    """U: the template argument launch_mha_encoder_bwd_mfma switches on."""
    return (key_tiles(N) + 7) // 8


def bwd_lds_bytes(N):
    """bwd_lds_bytes of encoder_attn_bwd_mfma.hip: KB and VB [NT][64][4], STAT [2][8][48], DQP [2][8][256], TR [8][16][20] floats."""
    return (key_tiles(N) * 512 + 2 * 8 * 48 + 2 * 8 * 256 + 8 * 16 * 20) * 4


def fwd_lds_bytes(N):
    """launch_mha_encoder_mfma: KF and VF [NT][64][4] floats."""
    return key_tiles(N) * 512 * 4


def fwd_kernel(N, key15=False):
    """The forward kernel the default dispatch takes above 127 nodes (E = 128, H = 8): mha_encoder_mfma_supports is
    NT * 2048 <= 150 KiB; debug key 15 keeps the tiled kernel."""
    return "mfma" if fwd_lds_bytes(N) <= 150 * 1024 and not key15 else "tiled"


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def _build():
    cs = []

    def case(name, N, kind, B=2, backward=True, dom=None):
        cs.append(dict(name=name, N=N, kind=kind, B=B, backward=backward, dom=dom))

    for N in BWD_NORMAL:
        case(f"normal_N{N}", N, "normal")
    for N in BWD_PEAKED:
        case(f"peaked_N{N}", N, "peaked")
    case("twin_N257", 257, "twin")
    for N, dom in BWD_DOMINANT:
        case(f"dominant_N{N}_k{dom}", N, "dominant", dom=dom)
    case("zero_rows_N385", 385, "zero_rows")
    for N in FWD_ONLY:
        case(f"fwd_normal_N{N}", N, "normal", B=1, backward=False)
    return {c["name"]: c for c in cs}


CASES = _build()
NAMES = list(CASES)
BACKWARD = [n for n in NAMES if CASES[n]["backward"]]


def outputs(c):
    """The outputs compared in case c."""
    return list(OUTPUTS if c["backward"] else OUTPUTS[:1])


def make_operands(kind, B, N, seed, dom=None):
    """-> dict(qkv [B, N, 384], dout [B, N, 128]) of data kind `kind`: float32 CPU tensors from the generator seeded `seed`."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, N, 3 * E, generator=g) * AMP[kind]
    dout = torch.randn(B, N, E, generator=g)
    if kind == "twin":
        qkv[:, N - 2] = qkv[:, 0]
    if kind == "dominant":
        u = torch.randn(B, 1, H, D, generator=g)
        u = (u / u.norm(dim=-1, keepdim=True) * math.sqrt(DOMINANT_GAP * math.sqrt(D))).reshape(B, 1, E)
        qkv[..., :E] += u
        qkv[:, dom, E:2 * E] += u[:, 0]
    if kind == "zero_rows":
        dout[:, list(ZERO_ROWS)] = 0.0
    return dict(qkv=qkv, dout=dout)


def operands(name):
    c = CASES[name]
    return make_operands(c["kind"], c["B"], c["N"], 3000 + NAMES.index(name), c["dom"])


def run_restatement(op, dtype, **kw):
    """-> dict of the restatement's outputs in `dtype`: y, and dqkv as its column blocks dq | dk | dv."""
    y, dqkv = tr.attention_backward(op["qkv"], op["dout"], H, dtype, **kw)
    return dict(y=y, dq=dqkv[..., :E], dk=dqkv[..., E:2 * E], dv=dqkv[..., 2 * E:])


def split(y, dqkv):
    """The kernels' outputs under the names of the restatement's."""
    return dict(y=y, dq=dqkv[..., :E], dk=dqkv[..., E:2 * E], dv=dqkv[..., 2 * E:])


def weights(op):
    """The float64 softmax weights [B, H, N, N] of the operands."""
    B, N, _ = op["qkv"].shape
    q, k = (op["qkv"].double()[..., i * E:(i + 1) * E].reshape(B, N, H, D).permute(0, 2, 1, 3) for i in range(2))
    return torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D), -1)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (op, r64, r32): the operands, the float64 and the float32 run of the restatement; r64["_scale"] holds max |output|.
    Computed once; nothing may modify it."""
    op = operands(name)
    r64, r32 = run_restatement(op, torch.float64), run_restatement(op, torch.float32)
    r64["_scale"] = {k: float(r64[k].abs().max()) for k in OUTPUTS}
    return op, r64, r32


def error(name, got, r64):
    """The error figure of output `name`: max-abs for y, the norm of the difference for a gradient block."""
    d = got.double() - r64[name]
    return float(d.abs().max()) if name == "y" else float(d.norm())


def bound(c, name, r64, r32):
    """-> (kind, bound) of output `name` of case c; kind: "maxabs" or "norm"."""
    scale = max(error(name, r32[name], r64), U * r64["_scale"][name])
    return ("maxabs" if name == "y" else "norm"), MARGIN * RATIO.get((name, c["kind"]), 1.0) * scale


def misses(c, got, r64, r32, names=None):
    """[(output, kind, figure, bound)] of the compared outputs of `got` that lie beyond their bound."""
    bad = []
    for name in names or outputs(c):
        kind, bd = bound(c, name, r64, r32)
        fig = error(name, got[name], r64)
        if not fig <= bd:
            bad.append((name, kind, fig, bd))
    return bad


def planted(name, which):
    """-> (the float64 outputs of case `name` with a deliberate error, the outputs the error reaches), or None where the case has no
    room for it (zero_rows_N385: the last query tile is the one row N - 1, whose dout is zero: it adds nothing to dk and dv):
      last_key_dropped          key N - 1 is not attended to
      last_key_tile_dropped     nor is any key of the last 16-key tile
      wave7_key_tiles_dropped   the key tiles kt = 7 (mod 8), one wave's share of the backward, are not attended to
      last_query_tile_skipped   the queries of the last 16-row tile are left out of dk and dv; y and dq are untouched by construction"""
    c = CASES[name]
    op, _, _ = reference(name)
    N = c["N"]
    assert which in PLANTS
    if which == "last_query_tile_skipped":
        if float(op["dout"][:, (N - 1) // 16 * 16:].abs().max()) == 0.0:
            return None
        return run_restatement(op, torch.float64, skip_queries=list(range((N - 1) // 16 * 16, N))), ("dk", "dv")
    if which == "last_key_dropped":
        keys = N - 1
    elif which == "last_key_tile_dropped":
        keys = (N - 1) // 16 * 16
    else:
        keys = (torch.arange(N) // 16) % 8 != 7
    return run_restatement(op, torch.float64, keys=keys), OUTPUTS
