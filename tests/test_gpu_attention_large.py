"""The three encoder self-attention kernels of the graphs above 112 nodes -- k_mha_encoder_mfma (forward, 128 .. 1200 nodes),
k_mha_encoder_tiled (the VALU forward: above 1200 nodes, and under debug key 15) and k_mha_encoder_bwd_mfma<U> (backward,
113 .. 1024 nodes, U = 1 .. 8) -- through ops.mha_encoder / ops.mha_encoder_backward:

  - every output on its own (y, and the column blocks dq | dk | dv of dqkv) against the float64 run of the restatement
    (tests/train_ref.py), with the cases, data kinds and bounds of tests/attn_large_cases.py: both sides of every U step, of the
    64 KiB LDS attribute of either MFMA kernel and of the forward's 1200-node limit, a peaked softmax, twin nodes, one dominant key
    in a padded last tile / in key 0 / in wave 7's first tile, zero rows of dout;
  - two runs bit-equal; dq of zero dout rows exactly zero; head 0 bit-identical when the other heads' data change;
  - the forward bit for bit against the oracle at every NT % 4, both LDS regimes, the 1200 | 1201 hand-over and 1281 nodes, through
    the default dispatch and through the tiled kernel (debug key 15);
  - the support surface of the backward.

Measured on the MI355X, kernel error / error of the restatement's float32 run, the largest over the cases per output and data
kind, and the case it occurs in (37 cases, 128 figures; the floor of tests/attn_large_cases.py was the larger scale in none):
  normal     y   3.33  normal_N897             dq  0.92  normal_N113          dk  1.51  normal_N897            dv  1.48  normal_N1023
             y above 1024 nodes (forward only): 2.27  fwd_normal_N1281 (k_mha_encoder_tiled by default dispatch; 2.20 at 1200, MFMA)
  peaked     y   1.00  peaked_N129             dq  1.03  peaked_N129          dk  1.04  peaked_N129            dv  1.00  peaked_N1024
  twin       y   0.96  twin_N257               dq  0.85  twin_N257            dk  1.13  twin_N257              dv  1.12  twin_N257
  dominant   y   2.63  dominant_N897_k115      dq  1.41  dominant_N273_k272   dk  2.08  dominant_N273_k272     dv  2.29  dominant_N1024_k1023
  zero_rows  y   0.91  zero_rows_N385          dq  0.80  zero_rows_N385       dk  1.18  zero_rows_N385         dv  1.16  zero_rows_N385
Every output stays inside the margin of 4 and tests/attn_large_cases.py records no RATIO.  The highest figures are y on the normal
data, where the ratio grows with the graph (1.2 at 113 nodes, 1.1 .. 1.7 to 513, 1.6 .. 3.3 from 640 on): the forward's value sum
is one fma chain over the keys in ascending order (the canonical order it shares bit for bit with the oracle), the restatement's a
blocked matrix product; the figure is the largest of 2 x N x 128 entries.  All eight instantiations of the backward ran (U = 1 .. 8:
the sizes of test_host_attention_large.py), both LDS regimes of either MFMA kernel, and k_mha_encoder_tiled at every size.
A second run, in another process, gave the same 128 figures to every printed digit; within one process two launches were bit-equal
in every output of every case (test_attention_kernels_are_deterministic).  The forward was bit-equal to the oracle in all 76
(data kind, size) pairs, through either kernel.
The 1281-node cases exposed a defect of the dispatch, not of a kernel: launch_mha_encoder refused every graph whose K and V exceed
160 KiB for ONE head (N > 1280) before choosing a kernel, although only its last resort, k_mha_encoder<D>, keeps them whole in LDS;
k_mha_encoder_tiled has no such limit.  The check now stands in front of that kernel alone.
"""
import numpy as np
import pytest
import torch

import attn_large_cases as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"


def run_kernels(op, backward=True):
    """-> dict of the kernels' outputs for the operands `op` (CPU tensors)."""
    from eam_rl4co_amd import ops

    qkv = op["qkv"].to(DEV).contiguous()
    y = ops.mha_encoder(qkv, ac.H)
    if backward:
        assert ops.mha_encoder_backward_supported(qkv.shape[1], ac.E, ac.H)
        got = ac.split(y, ops.mha_encoder_backward(qkv, op["dout"].to(DEV).contiguous(), ac.H))
    else:
        got = dict(y=y)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in got.items()}


@pytest.mark.parametrize("name", ac.NAMES)
def test_attention_kernels_match_the_float64_restatement(name):
    c = ac.CASES[name]
    op, r64, r32 = ac.reference(name)
    got = run_kernels(op, c["backward"])
    assert sorted(got) == sorted(ac.outputs(c))
    for k in ac.outputs(c):                     # each figure before any assert
        kind, bd = ac.bound(c, k, r64, r32)
        fig, f32 = ac.error(k, got[k], r64), ac.error(k, r32[k], r64)
        print(f"ATTNL {name} {k} {kind} kernel {fig:.3e} float32-restatement {f32:.3e} ratio {fig / f32 if f32 else float('nan'):.2f} "
              f"bound {bd:.3e} floor {ac.U * r64['_scale'][k]:.3e} ref {float(r64[k].norm()):.3e} "
              f"U {ac.bwd_tiles_per_wave(c['N'])} fwd {ac.fwd_kernel(c['N'])}")
    assert all(torch.isfinite(got[k]).all() for k in got)
    if c["kind"] == "zero_rows":                # dP = 0, X = 0, Delta = 0, dS = P * 0: exactly zero, in every head
        assert (got["dq"][:, list(ac.ZERO_ROWS)] == 0).all()
    assert ac.misses(c, got, r64, r32) == []


@pytest.mark.parametrize("name", ac.NAMES)
def test_attention_kernels_are_deterministic(name):
    """Two runs are bit-equal in every output: no atomics, every sum in a fixed order (the header of encoder_attn_bwd_mfma.hip)."""
    c = ac.CASES[name]
    op = ac.operands(name)
    a, b = run_kernels(op, c["backward"]), run_kernels(op, c["backward"])
    for k in ac.outputs(c):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


@pytest.mark.parametrize("name", ac.BACKWARD)
def test_heads_do_not_reach_each_other(name):
    """One workgroup per (instance, head): with heads 1 .. 7 of q, k, v and dout overwritten by other data, head 0's 16 columns of
    y, dq, dk and dv keep their bits."""
    op = ac.operands(name)
    a = run_kernels(op)
    g = torch.Generator().manual_seed(77)
    qkv, dout = op["qkv"].clone(), op["dout"].clone()
    for blk in range(3):
        qkv[..., blk * ac.E + ac.D:(blk + 1) * ac.E] = torch.randn(*qkv.shape[:2], ac.E - ac.D, generator=g) * 3.0
    dout[..., ac.D:] = torch.randn(*dout.shape[:2], ac.E - ac.D, generator=g) * 3.0
    b = run_kernels(dict(qkv=qkv, dout=dout))
    for k in ac.OUTPUTS:
        assert torch.equal(a[k][..., :ac.D].contiguous().view(torch.int32), b[k][..., :ac.D].contiguous().view(torch.int32)), k
        assert not torch.equal(a[k][..., ac.D:], b[k][..., ac.D:]), k


def _assert_bits_equal(a, b, what):
    a, b = a.detach().cpu().numpy(), np.asarray(b)
    assert a.shape == b.shape
    same = (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))      # (the sign of a zero carries no information)
    if not same.all():
        idx = np.argwhere(~same)[:5]
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} elements differ, first at {idx.tolist()}: "
                             f"{a[tuple(idx[0])]!r} vs {b[tuple(idx[0])]!r}")


@pytest.mark.parametrize("N", ac.ORACLE_SIZES)
@pytest.mark.parametrize("kind", ac.ORACLE_KINDS)
def test_forward_is_the_oracle_bit_for_bit(oracle, kind, N):
    """ops.mha_encoder against oracle.mha_encoder through the default dispatch (k_mha_encoder_mfma to 1200 nodes,
    k_mha_encoder_tiled above) and, to 1200 nodes, again with debug key 15 set (k_mha_encoder_tiled)."""
    from eam_rl4co_amd import _lib, ops

    B = 2 if N <= 193 else 1
    op = ac.make_operands(kind, B, N, 5000 + 4 * N + ac.ORACLE_KINDS.index(kind), dom=N - 1)
    ref = oracle.mha_encoder(op["qkv"].numpy(), ac.H)
    assert np.isfinite(ref).all()
    qkv = op["qkv"].to(DEV)
    _assert_bits_equal(ops.mha_encoder(qkv, ac.H), ref, f"default dispatch ({ac.fwd_kernel(N)})")
    if ac.fwd_kernel(N) == "mfma":
        lib = _lib.load()
        lib.eamrl_debug_set(15, 1)
        try:
            y = ops.mha_encoder(qkv, ac.H)
            torch.cuda.synchronize()
        finally:
            lib.eamrl_debug_set(15, 0)
        _assert_bits_equal(y, ref, "debug key 15 (tiled)")


def test_support_surface_of_the_backward():
    from eam_rl4co_amd import ops

    assert ops.mha_encoder_backward_supported(1024, ac.E, ac.H) and not ops.mha_encoder_backward_supported(1025, ac.E, ac.H)
    # the ABI's alignment REQUIRE: a contiguous qkv whose storage starts one float into its buffer
    B, N = 1, 113
    buf = torch.zeros(B * N * 3 * ac.E + 4, device=DEV)
    dout = torch.zeros(B, N, ac.E, device=DEV)
    for off in (1, 2, 3):
        qkv = buf[off:off + B * N * 3 * ac.E].view(B, N, 3 * ac.E)
        assert qkv.is_contiguous() and qkv.storage_offset() % 4 != 0
        with pytest.raises(RuntimeError, match="eamrl_mha_encoder_backward"):
            ops.mha_encoder_backward(qkv, dout, ac.H)
    torch.cuda.synchronize()
    aligned = buf[4:4 + B * N * 3 * ac.E].view(B, N, 3 * ac.E)
    assert bool((ops.mha_encoder_backward(aligned, dout, ac.H) == 0).all())      # (zero dout: a zero gradient)
