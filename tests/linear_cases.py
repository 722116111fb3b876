"""The cases of the linear launcher's tests (tests/test_host_linear.py on the CPU, tests/test_gpu_linear.py on the GPU): named
calls of ops.linear / ops.matmul_right, one or more for every kernel instantiation launch_linear (csrc/encoder.hip) can pick and
for every condition its dispatch (linear_variant) tests, each with the operand layout that condition is about.  The protocol is
that of tests/train_cases.py: the cases, their operands from a seeded generator, the reference computed once per case and shared,
the comparator, and the planted errors the comparator must reject.

A case records
  entry                 "linear" (eamrl_linear), "linear_bn" (eamrl_linear_bn) or "matmul_right" (eamrl_matmul_right)
  rows, in_dim, out_dim
  bias, relu, res, bn   which of the optional parts the call has
  x, W, y, resw         (ld, off): the leading dimension of the operand's rows and the element offset of its first element from
                        a 16-byte-aligned base.  off % 4 != 0 is a misaligned operand; ld > dim with off + dim <= ld is a column
                        window of a wider tensor (for W: the w_cols= argument), a plane of the slot-major cache for y
  bias_off              the same offset for the bias vector
  keys                  the debug keys set to 1 for the call
  variant               the name of the EAMRL_LINEAR_* id the dispatch must answer (written down from the conditions, not recorded
                        from a run)

The buffers.  Every operand is a window of a larger flat buffer: PAD elements, then `off`, then rows x ld, then PAD.
  inputs   NaN everywhere outside the window.  The kernels read in_dim columns of existing (or clamped) rows only, so the
           reference does not see the gaps; a kernel that lets one gap element reach a stored value stores a NaN.
  output   SENTINEL (an int32 that is no float a kernel could store: a NaN with a payload) everywhere.  After the call the whole
           buffer is compared as int32 with image(case): the reference's bits inside the window, SENTINEL everywhere else.  A
           16-byte store one lane too far, into the neighbouring plane, is a changed sentinel.

The reference is the oracle (oracle/eamrl_oracle.c) on contiguous copies of the windows: oracle.linear or oracle.matmul_right,
then res + v in float32, then oracle.batchnorm_eval -- the order of the kernels' epilogue.  Bits are compared as they are: no
zero of these cases is anything but the +0 a ReLU stores.

Shapes are the smallest that cross each edge.  The VALU causes other than in_dim % 32 stand at in_dim 64, so that each is the only
reason the call leaves the MFMA path (at in_dim 40 none of them would be alone); valu_all_strided_k40 has them together at the
shape with partial tiles in all three dimensions.
"""
import functools
import zlib

import numpy as np

PAD = 64                                   # elements before and after every window (a multiple of 4: the base stays aligned)
SENTINEL = np.int32(0x7FA5C3E1)            # a signalling NaN with a payload
EPS = 1e-5
THIN_MAX = 16384                           # k_thin_linear: rows * out_dim <= THIN_MAX
LD_MAX = (2 ** 31 - 1 - 124) // 127        # the largest ldx / ldw whose 128-row tile fits the MFMA kernel's 32-bit offsets
PLANTS = ("gap_overwritten", "last_row_clamped", "last_k_tile_dropped", "tail_columns_unwritten", "nan_stored")

# include/eamrl.h: EAMRL_LINEAR_<name>
VARIANTS = dict(NONE=0, SMALL4_K2=1, SMALL4_K3=2, SMALL4_K4=3, SMALL=4, THIN=5, VALU=6, MFMA64_EPI0=7, MFMA64_EPI1=8,
                MFMA64_EPI2=9, MFMA64_EPI3=10, MFMA64_RT=11, MFMA64_WT_EPI0=12, MFMA64_WT_RT=13, MFMA128_RT=14, MFMA128_WT_RT=15)
MFMA = frozenset(n for n in VARIANTS if n.startswith("MFMA"))


def _build():
    cs = []

    def case(name, variant, rows, in_dim, out_dim, *, entry=None, bias=None, relu=False, res=False, bn=False, x=None, W=None,
             y=None, resw=None, bias_off=0, keys=()):
        if entry is None:
            entry = "linear_bn" if bn else "linear"
        wt = entry == "matmul_right"
        if bias is None:
            bias = not wt
        c = dict(name=name, variant=variant, entry=entry, rows=rows, in_dim=in_dim, out_dim=out_dim, bias=bias, relu=relu,
                 res=res, bn=bn, x=x or (in_dim, 0), W=W or ((out_dim if wt else in_dim), 0), y=y or (out_dim, 0),
                 resw=(resw or (out_dim, 0)) if res else None, bias_off=bias_off, keys=tuple(keys))
        assert variant in VARIANTS and c["x"][0] >= in_dim and c["y"][0] >= out_dim and (not res or c["resw"][0] >= out_dim)
        if wt:            # ops.matmul_right: Wt contiguous, no bias / relu / residual / batch-norm
            assert c["W"][0] == out_dim and not (bias or relu or res or bn)
        else:             # ops.linear: W[:, w_cols] is a column window of a [out_dim, ldw] tensor
            assert c["W"][1] + in_dim <= c["W"][0] and not (relu and bn)
        assert all(c["name"] != name for c in cs)
        cs.append(c)

    mm = dict(entry="matmul_right")

    # ---- in_dim <= 4: k_small_linear4<K> (bias-only, aligned, four outputs per store) or k_small_linear ---------------------------
    for k, v in ((1, "SMALL"), (2, "SMALL4_K2"), (3, "SMALL4_K3"), (4, "SMALL4_K4")):
        case(f"small_k{k}", v, 5, k, 128)
    # the four-wide kernel on strided operands: odd x rows, an odd w_cols window, y the middle plane of a [rows, 3 * 128] buffer
    for k, v in ((2, "SMALL4_K2"), (3, "SMALL4_K3"), (4, "SMALL4_K4")):
        case(f"small_k{k}_strided", v, 5, k, 128, x=(k + 3, 1), W=(k + 5, 1), y=(384, 128), bias=(k != 3))
    # each condition of the four-wide kernel knocked out alone
    case("small_k3_out6", "SMALL", 5, 3, 6)
    case("small_k3_ldy130", "SMALL", 5, 3, 128, y=(130, 0))
    case("small_k3_y_off1", "SMALL", 5, 3, 128, y=(132, 1))
    case("small_k3_bias_off1", "SMALL", 5, 3, 128, bias_off=1)
    case("small_k3_relu", "SMALL", 5, 3, 128, relu=True)
    case("small_k3_res", "SMALL", 5, 3, 128, res=True)
    case("small_k3_bn", "SMALL", 5, 3, 128, bn=True)
    case("small_k3_wt", "SMALL", 5, 3, 128, **mm)
    case("small_k3_key0", "SMALL", 5, 3, 128, keys=(0,))
    case("small_k4_all_strided", "SMALL", 5, 4, 130, res=True, bn=True, x=(7, 1), W=(9, 3), y=(133, 2), resw=(131, 1), bias_off=3)

    # ---- k_thin_linear: rows * out_dim <= 16384, and the first shape beyond it ----------------------------------------------------
    for k in (5, 129, 32):
        case(f"thin_128x128_k{k}", "THIN", 128, k, 128)
        case(f"thin_128x128_k{k}_wt", "THIN", 128, k, 128, y=(131, 1), x=(k + 3, 1), **mm)
    case("thin_129x128_k5", "VALU", 129, 5, 128)
    case("thin_129x128_k129", "VALU", 129, 129, 128)
    case("thin_129x128_k32", "MFMA64_EPI0", 129, 32, 128)
    case("thin_129x128_k32_wt", "MFMA64_WT_EPI0", 129, 32, 128, **mm)
    case("thin_129x128_k5_wt", "VALU", 129, 5, 128, **mm)
    case("thin_all_strided_k5", "THIN", 128, 5, 128, res=True, bn=True, x=(8, 1), W=(9, 2), y=(130, 1), resw=(129, 3), bias_off=1)
    case("thin_all_strided_k129", "THIN", 127, 129, 129, relu=True, res=True, x=(132, 1), W=(131, 1), y=(131, 1), resw=(130, 3),
         bias_off=1)
    case("thin_key0", "VALU", 128, 32, 128, keys=(0,))

    # ---- k_linear_valu: each reason alone at rows 130, out_dim 132 ----------------------------------------------------------------
    case("valu_k40", "VALU", 130, 40, 132)
    case("valu_ldx66", "VALU", 130, 64, 132, x=(66, 0), relu=True)
    case("valu_x_off1", "VALU", 130, 64, 132, x=(68, 1), res=True)
    case("valu_ldw66", "VALU", 130, 64, 132, W=(66, 0), res=True, bn=True)
    case("valu_w_off1", "VALU", 130, 64, 132, W=(68, 1))
    case("valu_wt_out130", "VALU", 130, 64, 130, **mm)
    case("valu_key0", "VALU", 130, 64, 132, keys=(0,), bn=True)
    case("valu_wt_w_off1", "VALU", 130, 64, 132, W=(132, 1), **mm)
    case("valu_all_strided_k40", "VALU", 130, 40, 132, relu=True, res=True, x=(43, 1), W=(45, 3), y=(135, 1), resw=(133, 2),
         bias_off=1)

    # ---- k_linear_mfma<false, 64, EPI>, EPI 0 .. 3: windows of wider buffers, all 4-aligned ---------------------------------------
    epi = (dict(), dict(relu=True), dict(res=True), dict(res=True, bn=True))
    i = 0
    for rows in (129, 192):                # 129: the last row tile holds one row
        for out in (128, 256):
            for k in (32, 64, 96):         # 32: the k loop never prefetches
                e = i % 4
                case(f"mfma64_epi{e}_r{rows}_o{out}_k{k}", f"MFMA64_EPI{e}", rows, k, out, x=(3 * k, k), W=(2 * k, k),
                     y=(3 * out, out), resw=(3 * out, 2 * out), **epi[e])
                i += 1
    for e in range(4):                     # contiguous, no bias
        case(f"mfma64_epi{e}_plain", f"MFMA64_EPI{e}", 129, 64, 128, bias=False, **epi[e])

    # ---- k_linear_mfma<false, 64, -1>: each reason for the run-time epilogue alone ------------------------------------------------
    case("mfma64_rt_out132", "MFMA64_RT", 129, 64, 132)                       # a column tile of four columns
    case("mfma64_rt_out129", "MFMA64_RT", 129, 64, 129, res=True)             # scalar tail: one lane straddles out_dim
    case("mfma64_rt_out130", "MFMA64_RT", 129, 64, 130, relu=True)
    case("mfma64_rt_ldy130", "MFMA64_RT", 129, 64, 128, y=(130, 0))
    case("mfma64_rt_y_off1", "MFMA64_RT", 129, 64, 128, y=(132, 1))
    case("mfma64_rt_ldres130", "MFMA64_RT", 129, 64, 128, res=True, resw=(130, 0))
    case("mfma64_rt_res_off1", "MFMA64_RT", 129, 64, 128, res=True, resw=(132, 1))
    case("mfma64_rt_relu_res", "MFMA64_RT", 129, 64, 128, relu=True, res=True)
    case("mfma64_rt_bn_nores", "MFMA64_RT", 129, 64, 128, bn=True)
    case("mfma64_rt_key10", "MFMA64_RT", 129, 64, 128, keys=(10,))
    case("mfma64_rt_key10_res_bn", "MFMA64_RT", 192, 96, 256, res=True, bn=True, keys=(10,), x=(288, 96), W=(192, 96),
         y=(768, 256), resw=(768, 512))
    case("mfma64_rt_out132_planes", "MFMA64_RT", 129, 32, 132, res=True, bn=True, x=(96, 32), W=(64, 32), y=(396, 132),
         resw=(396, 264))                  # vec_ok per lane: the last 16-byte store ends where the next plane begins

    # ---- k_linear_mfma<true, 64, EPI>: eamrl_matmul_right ------------------------------------------------------------------------
    for k in (32, 64):
        case(f"wt_o128_k{k}", "MFMA64_WT_EPI0", 129, k, 128, x=(3 * k, k), y=(384, 128), **mm)
        case(f"wt_o132_k{k}", "MFMA64_WT_RT", 129, k, 132, x=(3 * k, k), y=(396, 132), **mm)       # second column tile: nvalid == 4
        case(f"wt_o256_k{k}", "MFMA64_WT_EPI0", 129, k, 256, x=(3 * k, k), y=(768, 256), **mm)
    case("wt_o128_y_off1", "MFMA64_WT_RT", 129, 64, 128, y=(132, 1), **mm)
    case("wt_o136_ldy138", "MFMA64_WT_RT", 129, 32, 136, y=(138, 0), **mm)                            # nvalid == 8
    case("wt_key10", "MFMA64_WT_RT", 129, 64, 128, keys=(10,), **mm)

    # ---- 128-row tiles (debug key 4) ------------------------------------------------------------------------------------------------
    case("mfma128_r129", "MFMA128_RT", 129, 64, 128, keys=(4,), res=True, bn=True)
    case("mfma128_r257_o132", "MFMA128_RT", 257, 32, 132, keys=(4,), relu=True, x=(96, 32), W=(64, 32), y=(396, 132))
    case("mfma128_wt_r129", "MFMA128_WT_RT", 129, 64, 128, keys=(4,), **mm)
    case("mfma128_wt_r257_o132", "MFMA128_WT_RT", 257, 32, 132, keys=(4,), x=(96, 32), y=(396, 132), **mm)

    # ---- edge row counts ----------------------------------------------------------------------------------------------------------
    case("rows0_linear", "NONE", 0, 64, 128, res=True)
    case("rows0_linear_bn", "NONE", 0, 3, 128, bn=True)
    case("rows0_matmul_right", "NONE", 0, 64, 128, **mm)
    case("rows1_thin", "THIN", 1, 64, 128, res=True, bn=True, y=(384, 128))
    case("rows1_small4", "SMALL4_K3", 1, 3, 128, y=(384, 128))
    case("rows1_valu", "VALU", 1, 64, 132, keys=(0,), y=(396, 132))
    return {c["name"]: c for c in cs}


CASES = _build()
NAMES = tuple(CASES)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def wt(c):
    return c["entry"] == "matmul_right"


def window(c, op):
    """(rows, cols, ld, off) of operand `op` ("x", "W", "y", "resw", "bias"): the window starts PAD + off elements into its buffer."""
    if op == "bias":
        return 1, c["out_dim"], c["out_dim"], c["bias_off"]
    ld, off = c[op]
    if op == "x":
        return c["rows"], c["in_dim"], ld, off
    if op == "W":
        return (c["in_dim"], c["out_dim"], ld, off) if wt(c) else (c["out_dim"], c["in_dim"], ld, off)
    return c["rows"], c["out_dim"], ld, off


def buffer_len(c, op):
    r, _, ld, off = window(c, op)
    return PAD + off + r * ld + PAD


def window_index(c, op):
    """Flat indices [rows, cols] of the window's elements in its buffer."""
    r, n, ld, off = window(c, op)
    return PAD + off + np.arange(r, dtype=np.int64)[:, None] * ld + np.arange(n, dtype=np.int64)[None, :]


def pointer(c, op, base):
    """A fake address with the operand's alignment (base: a multiple of 16)."""
    return base + 4 * (PAD + window(c, op)[3])


# ---- operands and reference -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def operands(name):
    """Contiguous float32 operands of a case: x [rows, in], W ([out, in], or [in, out] for matmul_right), bias, res, and the four
    batch-norm vectors (None where the case has none).  Treat as read-only."""
    c = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rows, k, n = c["rows"], c["in_dim"], c["out_dim"]
    op = dict(x=rng.standard_normal((rows, k)).astype(np.float32),
              W=(rng.standard_normal((k, n) if wt(c) else (n, k)) / np.sqrt(k)).astype(np.float32),
              bias=rng.standard_normal(n).astype(np.float32) if c["bias"] else None,
              resw=rng.standard_normal((rows, n)).astype(np.float32) if c["res"] else None,
              bn=None)
    if c["bn"]:
        op["bn"] = (rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32),
                    rng.standard_normal(n).astype(np.float32), (rng.random(n) + 0.5).astype(np.float32))
    for v in op.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if a is not None:
                a.setflags(write=False)
    return op


def input_buffer(name, op):
    """The flat float32 buffer of an input operand ("x", "W", "resw", "bias"): NaN outside the window."""
    c = CASES[name]
    buf = np.full(buffer_len(c, op), np.nan, np.float32)
    buf[window_index(c, op)] = np.atleast_2d(operands(name)[op])
    return buf


def output_buffer(name):
    """The flat int32 buffer the output is written into: SENTINEL everywhere."""
    return np.full(buffer_len(CASES[name], "y"), SENTINEL, np.int32)


def chain(name, k_used=None):
    """The oracle's k-ordered chain alone (bias + sum over k, no epilogue), on the first k_used columns."""
    from oracle import oracle as orc

    c, op = CASES[name], operands(name)
    k = c["in_dim"] if k_used is None else k_used
    if wt(c):
        return orc.matmul_right(op["x"][:, :k], op["W"][:k])
    return orc.linear(op["x"][:, :k], op["W"][:, :k], op["bias"])


def epilogue(name, v):
    """ReLU, then res + v in float32, then the eval batch-norm: the oracle's, in the kernels' order."""
    from oracle import oracle as orc

    c, op = CASES[name], operands(name)
    if c["relu"]:
        v = np.where(v > 0, v, np.float32(0.0)).astype(np.float32)
    if c["res"]:
        v = op["resw"] + v
    if c["bn"] and v.size:
        v = orc.batchnorm_eval(v[None], *op["bn"], eps=EPS)[0]
    assert v.dtype == np.float32
    return v


@functools.lru_cache(maxsize=None)
def reference(name):
    """[rows, out_dim] float32: the value every kernel variant must store, bit for bit.  Read-only."""
    from oracle import oracle as orc

    c, op = CASES[name], operands(name)
    if wt(c):
        v = orc.matmul_right(op["x"], op["W"])
    else:
        v = orc.linear(op["x"], op["W"], op["bias"], relu=c["relu"])
    if c["res"]:
        v = op["resw"] + v
    if c["bn"] and v.size:
        v = orc.batchnorm_eval(v[None], *op["bn"], eps=EPS)[0]
    assert v.dtype == np.float32 and v.shape == (c["rows"], c["out_dim"]) and np.isfinite(v).all()
    assert not np.signbit(v[v == 0]).any()           # the only zeros are the ReLU's +0: bits can be compared as they are
    assert np.array_equal(v.view(np.int32), epilogue(name, chain(name)).view(np.int32))       # what plant() builds on
    v.setflags(write=False)
    return v


def image(name, values=None):
    """The whole output buffer as int32 after a correct call: `values` (the reference by default) in the window, SENTINEL
    everywhere else."""
    buf = output_buffer(name)
    v = reference(name) if values is None else values
    buf[window_index(CASES[name], "y")] = np.ascontiguousarray(v, np.float32).view(np.int32)
    return buf


# ---- the comparator ---------------------------------------------------------------------------------------------------------------
def check_case(buffer, case):
    """buffer: the output buffer after the call, int32, whole.  Raises AssertionError unless the window holds the reference's bits
    and every other element still holds SENTINEL."""
    c = CASES[case] if isinstance(case, str) else case
    name = c["name"]
    got = np.asarray(buffer)
    assert got.dtype == np.int32 and got.shape == (buffer_len(c, "y"),), (got.dtype, got.shape)
    want = image(name)
    if np.array_equal(got, want):
        return
    inside = np.zeros(got.shape, bool)
    idx = window_index(c, "y")
    inside[idx] = True
    bad = got != want
    gaps = np.flatnonzero(bad & ~inside)
    msg = [f"{name} ({c['variant']}):"]
    if gaps.size:
        rel = gaps - (PAD + c["y"][1])
        msg.append(f"{gaps.size} elements outside the output window were written, first at buffer index {int(gaps[0])} "
                   f"(row {int(rel[0] // c['y'][0])}, column {int(rel[0] % c['y'][0])} of the ld-{c['y'][0]} rows)")
    wbad = np.argwhere(bad[idx])
    if wbad.size:
        r, j = (int(t) for t in wbad[0])
        g = got[idx[r, j]:idx[r, j] + 1].view(np.float32)[0]
        msg.append(f"{len(wbad)} of {idx.size} stored values differ from the oracle, first at [{r}, {j}]: "
                   f"{g!r} (0x{int(got[idx[r, j]]) & 0xffffffff:08x}) vs {reference(name)[r, j]!r}")
    raise AssertionError(" ".join(msg))


def plant(name, kind):
    """The output buffer a kernel with the named fault would leave (int32), built from the reference."""
    c = CASES[name]
    ref = reference(name)
    if kind == "gap_overwritten":                  # a store one element past the end of the first row
        assert c["y"][0] > c["out_dim"]
        buf = image(name)
        buf[PAD + c["y"][1] + c["out_dim"]] = np.float32(1.0).view(np.int32)
        return buf
    if kind == "last_row_clamped":                 # the clamped copy of a row stored in place of the row
        v = ref.copy()
        v[-1] = v[-2]
        return image(name, v)
    if kind == "last_k_tile_dropped":
        k = c["in_dim"]
        return image(name, epilogue(name, chain(name, k - (k % 32 or 32))))
    if kind == "tail_columns_unwritten":
        buf = image(name)
        buf[window_index(c, "y")[:, -4:]] = SENTINEL
        return buf
    if kind == "nan_stored":
        v = ref.copy()
        v[c["rows"] // 2, c["out_dim"] // 2] = np.nan
        return image(name, v)
    raise KeyError(kind)
