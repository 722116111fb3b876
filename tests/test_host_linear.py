"""CPU: the linear launcher's dispatch (eamrl_linear_variant: host arithmetic, no launch), the guards of its three entry points,
and the instruments of tests/test_gpu_linear.py -- the cases cover every instantiation, the comparator rejects the planted
faults, and the bit-exact reference is the right operation (the oracle's chain against a float64 matmul)."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

import linear_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
BASES = dict(x=0x10000000, W=0x20000000, bias=0x30000000, resw=0x40000000, y=0x50000000)      # never dereferenced


@pytest.fixture(scope="module")
def lib():
    from eam_rl4co_amd import _lib

    return _lib.load()


@contextlib.contextmanager
def debug_keys(lib, keys):
    for k in keys:
        assert lib.eamrl_debug_set(k, 1) == 0
    try:
        yield
    finally:
        for k in keys:
            lib.eamrl_debug_set(k, 0)


def variant_of(lib, c, extra_keys=(), **over):
    """eamrl_linear_variant on fake pointers that carry the case's alignment."""
    a = dict(ldx=c["x"][0], ldw=c["W"][0], ldres=c["resw"][0] if c["res"] else 0, ldy=c["y"][0], rows=c["rows"],
             in_dim=c["in_dim"], out_dim=c["out_dim"])
    a.update(over)
    p = {op: C.c_void_p(lc.pointer(c, op, BASES[op])) for op in ("x", "W", "y")}
    p["bias"] = C.c_void_p(lc.pointer(c, "bias", BASES["bias"])) if c["bias"] else None
    p["resw"] = C.c_void_p(lc.pointer(c, "resw", BASES["resw"])) if c["res"] else None
    with debug_keys(lib, tuple(c["keys"]) + tuple(extra_keys)):
        return lib.eamrl_linear_variant(p["x"], a["ldx"], p["W"], a["ldw"], int(lc.wt(c)), p["bias"], p["resw"], a["ldres"],
                                        p["y"], a["ldy"], a["rows"], a["in_dim"], a["out_dim"], int(c["relu"]), int(c["bn"]))


def test_header_declares_the_variant_ids_and_the_entry_point():
    from eam_rl4co_amd import _lib

    with open(os.path.join(ROOT, "include", "eamrl.h")) as f:
        text = f.read()
    defines = {k: int(v) for k, v in re.findall(r"#define\s+EAMRL_LINEAR_(\w+)\s+(\d+)", text)}
    assert defines == lc.VARIANTS
    assert len(set(defines.values())) == len(defines)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+eamrl_linear_variant\s*\(", code)
    assert len(_lib.PROTOTYPES["eamrl_linear_variant"]) == 15
    assert _lib.load().eamrl_version() == 101


def test_every_case_takes_its_recorded_variant(lib):
    got = {name: variant_of(lib, c) for name, c in lc.CASES.items()}
    wrong = {n: (v, lc.VARIANTS[lc.CASES[n]["variant"]]) for n, v in got.items() if v != lc.VARIANTS[lc.CASES[n]["variant"]]}
    assert not wrong, wrong
    # under debug key 0 nothing runs on the MFMA kernels: the GPU test's second run is the VALU kernel
    for name, c in lc.CASES.items():
        if c["variant"] in lc.MFMA:
            assert variant_of(lib, c, extra_keys=(0,)) == lc.VARIANTS["VALU"], name


def test_the_cases_reach_exactly_the_declared_variants():
    """A new instantiation with no case fails here; so does the removal of the only case of an id."""
    assert {c["variant"] for c in lc.CASES.values()} == set(lc.VARIANTS)
    assert {c["entry"] for c in lc.CASES.values()} == {"linear", "linear_bn", "matmul_right"}
    for v in lc.MFMA:          # every MFMA instantiation on strided operands, not only on contiguous ones
        assert any(c["variant"] == v and c["x"][0] > c["in_dim"] and c["y"][0] > c["out_dim"] for c in lc.CASES.values()), v


def test_the_cases_stand_on_the_edges_they_name():
    cs = lc.CASES
    assert cs["thin_128x128_k5"]["rows"] * cs["thin_128x128_k5"]["out_dim"] == lc.THIN_MAX
    assert cs["thin_129x128_k32"]["rows"] * cs["thin_129x128_k32"]["out_dim"] == lc.THIN_MAX + 128
    assert {c["in_dim"] for c in cs.values() if c["variant"].startswith("SMALL")} == {1, 2, 3, 4}
    epi = [c for c in cs.values() if c["variant"] in ("MFMA64_EPI0", "MFMA64_EPI1", "MFMA64_EPI2", "MFMA64_EPI3")]
    assert {(c["rows"], c["out_dim"], c["in_dim"]) for c in epi} >= {(r, o, k) for r in (129, 192) for o in (128, 256)
                                                                     for k in (32, 64, 96)}
    rt = {c["out_dim"] for c in cs.values() if c["variant"] == "MFMA64_RT"}
    assert rt >= {128, 129, 130, 132}
    assert {(c["rows"], lc.wt(c)) for c in cs.values() if 4 in c["keys"]} == {(129, False), (257, False), (129, True), (257, True)}
    assert {c["rows"] for c in cs.values()} >= {0, 1}
    # every operand is misaligned in some case and a window of a wider buffer in some case
    for op, dim in (("x", "in_dim"), ("y", "out_dim"), ("resw", "out_dim")):
        have = [c for c in cs.values() if c[op] is not None]
        assert any(c[op][1] % 4 for c in have) and any(c[op][0] % 4 for c in have) and any(c[op][0] >= 2 * c[dim] for c in have), op
    assert any(c["W"][1] % 4 for c in cs.values()) and any(c["W"][0] % 4 and not lc.wt(c) for c in cs.values())
    assert any(c["bias_off"] % 4 for c in cs.values())
    # no output larger than 257 x 256
    assert all(c["rows"] <= 257 and c["out_dim"] <= 256 for c in cs.values())


def test_leading_dimensions_beyond_32_bit_tile_offsets_leave_the_mfma_path(lib):
    """gemm_offsets forms row * ld + column in 32 bits, up to 127 * ld + 124: INT_MAX // 127 = 16909320 (a multiple of 4, so
    nothing else diverts it) already overflows with the column added."""
    assert lc.LD_MAX == 16909319 and 127 * lc.LD_MAX + 124 <= 2 ** 31 - 1 < 127 * (lc.LD_MAX + 1) + 124
    mf, wt_ = lc.CASES["mfma64_epi0_plain"], lc.CASES["wt_o256_k64"]
    ok = lc.LD_MAX // 4 * 4
    assert variant_of(lib, mf, ldx=ok, ldw=ok) == lc.VARIANTS["MFMA64_EPI0"]
    assert variant_of(lib, wt_, ldx=ok) == lc.VARIANTS["MFMA64_WT_EPI0"]
    for ld in (ok + 4, (2 ** 31 - 1) // 127 + 4, 2 ** 31, 2 ** 40):
        assert ld % 4 == 0
        assert variant_of(lib, mf, ldx=ld) == lc.VARIANTS["VALU"], ld
        assert variant_of(lib, mf, ldw=ld) == lc.VARIANTS["VALU"], ld
        assert variant_of(lib, wt_, ldx=ld) == lc.VARIANTS["VALU"], ld
        for key in (4, 10):
            assert variant_of(lib, mf, extra_keys=(key,), ldx=ld) == lc.VARIANTS["VALU"], (ld, key)
    # the transposed weight's leading dimension is out_dim: int at the ABI, but the rule is the same one
    big = lc.LD_MAX // 4 * 4 + 4
    assert variant_of(lib, wt_, out_dim=big, ldw=big, ldy=big) == lc.VARIANTS["VALU"]


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    p, q, r, s = (C.c_void_p(v) for v in (4096, 8192, 12288, 16384))        # never dereferenced: every call is rejected

    def rejected(fn, *args):
        assert getattr(lib, fn)(*args) == -1
        msg = lib.eamrl_last_error()
        assert fn.encode() + b": requirement failed" in msg, msg

    huge = 128 * 2 ** 31                         # (rows + 127) / 128 row tiles do not fit the grid
    # eamrl_linear(x, ldx, W, ldw, bias, res, ldres, y, ldy, rows, in_dim, out_dim, relu, stream)
    good = [p, 64, q, 64, None, None, 0, r, 128, 129, 64, 128, 0, None]
    bn = [s, s, s, s, C.c_float(1e-5), None]
    for i, v in ((0, None), (2, None), (7, None), (1, 63), (3, 63), (8, 127), (9, -1), (9, huge), (10, 0), (11, 0)):
        bad = list(good)
        bad[i] = v
        rejected("eamrl_linear", *bad)
        rejected("eamrl_linear_bn", *bad[:12], *bn)
    rejected("eamrl_linear", *good[:5], s, 127, *good[7:])                      # a residual with ldres < out_dim
    rejected("eamrl_linear_bn", *good[:12], None, s, s, s, C.c_float(1e-5), None)
    # eamrl_matmul_right(x, ldx, Wt, y, ldy, rows, in_dim, out_dim, stream)
    good = [p, 64, q, r, 128, 129, 64, 128, None]
    for i, v in ((0, None), (2, None), (3, None), (1, 63), (4, 127), (5, -1), (5, huge), (6, 0), (7, 0)):
        bad = list(good)
        bad[i] = v
        rejected("eamrl_matmul_right", *bad)
    # eamrl_linear_variant(x, ldx, W, ldw, wt, bias, res, ldres, y, ldy, rows, in_dim, out_dim, relu, bn): the same requirements
    good = [p, 64, q, 64, 0, None, None, 0, r, 128, 129, 64, 128, 0, 0]
    assert lib.eamrl_linear_variant(*good) == lc.VARIANTS["MFMA64_EPI0"]
    for i, v in ((0, None), (2, None), (8, None), (1, 63), (3, 63), (9, 127), (10, -1), (10, huge), (11, 0), (12, 0)):
        bad = list(good)
        bad[i] = v
        rejected("eamrl_linear_variant", *bad)
    wt_good = [p, 64, q, 128, 1, None, None, 0, r, 128, 129, 64, 128, 0, 0]
    assert lib.eamrl_linear_variant(*wt_good) == lc.VARIANTS["MFMA64_WT_EPI0"]
    wt_good[3] = 127                                                               # Wt rows are out_dim long
    rejected("eamrl_linear_variant", *wt_good)
    # an empty batch is accepted and launches nothing
    assert lib.eamrl_linear(p, 64, q, 64, None, None, 0, r, 128, 0, 64, 128, 0, None) == 0
    assert lib.eamrl_matmul_right(p, 64, q, r, 128, 0, 64, 128, None) == 0


def test_one_copy_of_the_dispatch_conditions():
    with open(os.path.join(ROOT, "eam_rl4co_amd", "csrc", "encoder.hip")) as f:
        text = f.read()
    assert text.count("g.rows * g.out_dim <= 16384") == 1 and text.count("g.in_dim % GK") == 1
    assert text.count("g_debug[10]") == 1 and text.count("g_debug[4]") == 1 and text.count("g_debug[0]") == 1
    launch = text[text.index("int launch_linear("):]
    launch = launch[:launch.index("\n}\n")]
    assert "linear_variant(g)" in launch and "uintptr_t" not in launch and "g_debug" not in launch
    assert launch.count("hipLaunchKernelGGL") == len(lc.VARIANTS) - 1            # one launch per id but NONE


# ---- the comparator ---------------------------------------------------------------------------------------------------------------
PLANT_CASES = ("mfma64_rt_out132_planes", "mfma64_epi3_r129_o256_k32", "wt_o132_k64", "thin_all_strided_k129", "small_k3_strided",
               "valu_all_strided_k40")


@pytest.mark.parametrize("name", PLANT_CASES)
def test_comparator_accepts_the_reference_and_rejects_every_planted_fault(oracle, name):
    c = lc.CASES[name]
    lc.check_case(lc.image(name), c)
    lc.check_case(lc.image(name), name)
    for kind in lc.PLANTS:
        buf = lc.plant(name, kind)
        assert not np.array_equal(buf, lc.image(name)), kind
        with pytest.raises(AssertionError, match=name):
            lc.check_case(buf, c)
    with pytest.raises(AssertionError, match="outside the output window"):
        lc.check_case(lc.plant(name, "gap_overwritten"), c)
    with pytest.raises(AssertionError, match="differ from the oracle"):
        lc.check_case(lc.plant(name, "last_row_clamped"), c)
    # an untouched buffer, and one written before the window's first element
    with pytest.raises(AssertionError):
        lc.check_case(lc.output_buffer(name), c)
    buf = lc.image(name)
    buf[lc.PAD + c["y"][1] - 1] = 0
    with pytest.raises(AssertionError, match="outside the output window"):
        lc.check_case(buf, c)


def test_the_132_wide_case_notices_its_four_tail_columns(oracle):
    name = "mfma64_rt_out132"
    c = lc.CASES[name]
    assert c["out_dim"] == 132
    buf = lc.plant(name, "tail_columns_unwritten")
    idx = lc.window_index(c, "y")
    assert (buf[idx[:, 128:]] == lc.SENTINEL).all() and np.array_equal(buf[idx[:, :128]], lc.image(name)[idx[:, :128]])
    with pytest.raises(AssertionError, match=rf"{4 * c['rows']} of {132 * c['rows']} stored values differ"):
        lc.check_case(buf, c)


def test_empty_cases_expect_an_untouched_buffer(oracle):
    for name in ("rows0_linear", "rows0_linear_bn", "rows0_matmul_right"):
        assert (lc.image(name) == lc.SENTINEL).all()
        lc.check_case(lc.output_buffer(name), name)


def test_input_buffers_hold_nan_outside_the_windows(oracle):
    for name in ("mfma64_epi3_r129_o256_k32", "valu_all_strided_k40", "wt_o132_k64"):
        c = lc.CASES[name]
        for op in ("x", "W", "resw", "bias"):
            if lc.operands(name)[op] is None:
                continue
            buf = lc.input_buffer(name, op)
            idx = lc.window_index(c, op)
            assert np.array_equal(buf[idx], np.atleast_2d(lc.operands(name)[op]))
            outside = np.ones(buf.shape, bool)
            outside[idx] = False
            assert np.isnan(buf[outside]).all() and outside.sum() >= 2 * lc.PAD
            assert lc.pointer(c, op, 4096) % 16 == (4 * lc.window(c, op)[3]) % 16


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in lc.NAMES if lc.CASES[n]["rows"] > 0])
def test_oracle_chain_is_the_matmul_within_the_rounding_of_a_chain(oracle, name):
    """|chain - exact| <= (in_dim + 2) 2^-24 sum |terms| per entry: in_dim + 1 roundings of the in_dim fma and the bias start
    (gamma_n = n u / (1 - n u) <= (n + 1) u at these n), against the float64 sum whose own error is 2^-29 of that."""
    c, op = lc.CASES[name], lc.operands(name)
    x = op["x"].astype(np.float64)
    W = op["W"].astype(np.float64) if lc.wt(c) else op["W"].astype(np.float64).T
    b = np.zeros(c["out_dim"]) if op["bias"] is None else op["bias"].astype(np.float64)
    want = x @ W + b
    terms = np.abs(x) @ np.abs(W) + np.abs(b)
    got = lc.chain(name).astype(np.float64)
    err = np.abs(got - want)
    bound = (c["in_dim"] + 2) * U * terms
    worst = float((err / bound).max())
    print(f"LINEAR_CHAIN {name}: max err / bound {worst:.3f}")
    assert (err <= bound).all(), worst
    # and the reference proper is that chain through the oracle's own ReLU, the float32 residual add and the oracle's batch-norm
    ref = lc.reference(name)
    v = got
    if c["relu"]:
        v = np.maximum(v, 0.0)
    if c["res"]:
        v = v + op["resw"].astype(np.float64)
    if c["bn"]:
        g, bt, mu, var = (a.astype(np.float64) for a in op["bn"])
        v = (v - mu) / np.sqrt(var + np.float64(np.float32(lc.EPS))) * g + bt
        scale = np.abs(g) / np.sqrt(var) * (np.abs(mu) + np.abs(got) + (np.abs(op["resw"]) if c["res"] else 0)) + np.abs(bt)
    else:
        scale = np.abs(v)
    # at most 8 float32 roundings past the chain (the add; scale: add, sqrt, divide; mean * scale; beta - that; the fma), each
    # relative to a term of `scale`
    assert (np.abs(ref.astype(np.float64) - v) <= 8 * U * scale).all()
