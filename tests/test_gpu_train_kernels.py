"""The kernels behind the differentiable encoder (eam_rl4co_amd/train.py: _LinearFn, _SmallLinearFn, _InstanceNormFn,
_BatchNormTrainFn, _self_attention up to 112 nodes) through eam_rl4co_amd.ops, every output tensor on its own against the float64
restatement of the operation (tests/train_ref.py).  The cases, their data kinds and their bounds are those of
tests/train_cases.py; what each group is there for:

  lin_*   ops.linear_wgrad: one chunk with ragged slabs, 2 / 4 / 13 / 17 chunks with a last chunk of one row, grids with x > 1
          and y > 1 (the bias from blockIdx.y == 0 only), the capped chunking with empty trailing chunks (32 and 512 chunks),
          column slices of wider tensors, need_bias=False; the chunk count of every case is asserted against the library's
  sm_*    ops.small_linear_wgrad: every K from 1 to 8, both sides of the 256-row chunk, out_dim 64 / 100 / 128 / 300 (the guard
          o < out_dim, the strided o loop), a strided x and a strided dy, need_bias=False
  in_*    ops.instance_norm_forward / _backward: N below the backward's four row groups, both sides of the 64 KiB and 96 KiB edges
          of the forward's LDS tile and the global-memory walk beyond, E = 6 .. 300 (scalar staging, the channel loops), 600
          instances on the dgamma / dbeta atomics, need_affine_grads=False; y bit-equal to ops.normalize_ (the rollout's
          k_norm_instance) in every case
  bn_*    ops.batchnorm_backward on the float32-rounded float64 statistics: rows = 1 (dx exactly 0), the 128-row chunk edges, the
          grid-stride second trip of k_bn_bwd_dx, E up to 2048 (the channel loop at 1024 threads), need_affine_grads=False
  at_*    ops.mha_encoder / ops.mha_encoder_backward at both sides of every key tile and of the 32 / 64 / 112-key kernels, a
          peaked softmax (amplitude 6), two bit-identical nodes
  *_offset, *_const, *_tiny    the data kinds of tests/train_cases.py

Measured on the MI355X, kernel error / error of the restatement's float32 run, the largest over the 103 cases per output (cases
in which the float32 run is exact left aside: the floor of tests/train_cases.py bounds them), and the case it occurs in:
  linear   dW      1.00  lin_r1_128x128            db     25.09  lin_r193_128x128_offset  (1.71 on the normal data, lin_r64_128x128)
  small    dW      1.08  sm_r257_K3_o64            db      3.17  sm_r257_K1_o128
  instnorm y       1.84  in_B3_N300_E128           mean    3.61  in_B3_N300_E128          rstd    2.74  in_B3_N191_E128
           dx      1.84  in_B3_N300_E128           dgamma  3.04  in_B600_N20_E128         dbeta   3.15  in_B600_N20_E128
  bn       dx      1.06  bn_r129_E128_noaux        dgamma  2.26  bn_r129_E128_noaux       dbeta   2.47  bn_r127_E128
  attn     y       1.31  at_N17_a1.5               dqkv    1.05  at_N112_a1.5
A second run gave the same bits in 304 of the 333 figures; the 29 others are dgamma / dbeta of the instance norm over more than one
instance (float atomics: the order differs from run to run), which moved by up to 0.44: 2.60 and 3.37 at in_B600_N20_E128 in the
other run.  In that case the floor is the larger scale (600 x 20 terms per channel): the kernel's error is 1.28 and 0.90 times it.
Every output stays inside the margin of 4 except the bias gradient of ops.linear_wgrad on the offset data, by rounding and not by
a defect: the kernel sums the rows of each parity apart, so the alternating signs cancel only at the end, where the restatement's
sum in row order cancels at every step (train_cases.RATIO has the arithmetic).  Against the scale that bounds it -- the floor
there, U sum |terms| -- it is 7.21 (lin_r66_128x128_offset) and 6.09 (lin_r193_128x128_offset): its bound is the recorded ratio
7.21 with the same margin.  The highest of the others are sequential float32 sums over 300 nodes / 257 rows against torch's
blocked sums (mean, db); an emulation of the kernel's order on the CPU gives the same 3.61 for the mean at N = 300.  The forward's
y was bit-equal to ops.normalize_ in all three regimes of k_instnorm_train_fwd, E % 4 != 0 included.
"""
import pytest
import torch

import train_cases as tc

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _wide(t, left, right):
    """t as a column slice of a wider tensor on the GPU."""
    w = torch.full((t.shape[0], left + t.shape[1] + right), 7.0, device=DEV)
    w[:, left:left + t.shape[1]] = t.to(DEV)
    return w[:, left:left + t.shape[1]]


def run_kernels(name):
    """-> dict of the kernels' outputs for case `name` (CPU tensors), the exact-equality properties of the case asserted on the way."""
    from eam_rl4co_amd import _lib, ops

    c = tc.CASES[name]
    op, r64, _ = tc.reference(name)
    fam = c["fam"]
    dev = {k: v.to(DEV).contiguous() for k, v in op.items()}
    if fam in ("linear", "small"):
        dy, x = dev["dy"], dev["x"]
        if c["strided"] in ("both", "dy"):
            dy = _wide(op["dy"], 128, 0)
        if c["strided"] in ("both", "x"):
            x = _wide(op["x"], 128, 128) if fam == "linear" else _wide(op["x"], 0, 2)
        assert c["strided"] is None or dy.stride(0) != dy.shape[1] or x.stride(0) != x.shape[1]
        if fam == "linear":
            per_chunk = c["out"] * c["inp"] + c["out"]
            need = _lib.load().eamrl_linear_wgrad_scratch(c["rows"], c["out"], c["inp"])
            assert need % per_chunk == 0 and need // per_chunk == c["nch"], (need // per_chunk, c["nch"])
        fn = ops.linear_wgrad if fam == "linear" else ops.small_linear_wgrad
        dW, db = fn(dy, x)
        if c["no_aux"]:
            dW2, none = fn(dy, x, need_bias=False)
            assert none is None and torch.equal(dW2, dW)
        got = dict(dW=dW, db=db)
    elif fam == "instnorm":
        y, mean, rstd = ops.instance_norm_forward(dev["x"], dev["gamma"], dev["beta"], tc.EPS)
        # the "same arithmetic" claim of csrc/encoder.hip: bit-equal to the rollout's in-place kernel, in all three regimes
        y2 = ops.normalize_(dev["x"].clone(), ops.NORM_INSTANCE, dev["gamma"], dev["beta"], eps=tc.EPS)
        assert torch.equal(y, y2), tc.instnorm_lds(c["N"], c["E"])
        dx, dg, db = ops.instance_norm_backward(dev["x"], dev["dy"], mean, rstd, dev["gamma"])
        if c["no_aux"]:
            dx2, n1, n2 = ops.instance_norm_backward(dev["x"], dev["dy"], mean, rstd, dev["gamma"], need_affine_grads=False)
            assert n1 is None and n2 is None and torch.equal(dx2, dx)
        got = dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dg, dbeta=db)
    elif fam == "bn":
        dx, dg, db = ops.batchnorm_backward(dev["x"], dev["dy"], dev["mean"], dev["var"], dev["gamma"], tc.EPS)
        if c["no_aux"]:
            dx2, n1, n2 = ops.batchnorm_backward(dev["x"], dev["dy"], dev["mean"], dev["var"], dev["gamma"], tc.EPS,
                                                 need_affine_grads=False)
            assert n1 is None and n2 is None and torch.equal(dx2, dx)
        got = dict(dx=dx, dgamma=dg, dbeta=db)
    else:
        assert ops.mha_encoder_backward_supported(c["N"], tc.E_ATT, tc.H)
        got = dict(y=ops.mha_encoder(dev["qkv"], tc.H), dqkv=ops.mha_encoder_backward(dev["qkv"], dev["dout"], tc.H))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in got.items()}


@pytest.mark.parametrize("name", tc.NAMES)
def test_training_kernels_match_the_float64_restatement(name):
    c = tc.CASES[name]
    op, r64, r32 = tc.reference(name)
    got = run_kernels(name)
    assert sorted(got) == sorted(tc.outputs(c))
    for k in tc.outputs(c):                     # each figure before any assert
        kind, bd = tc.bound(c, k, r64, r32)
        fig, f32 = tc.error(k, got[k], r64), tc.error(k, r32[k], r64)
        print(f"TRAINK {name} {k} {kind} kernel {fig:.3e} float32-restatement {f32:.3e} ratio {fig / f32 if f32 else float('nan'):.2f} "
              f"bound {bd:.3e} floor {tc.U * r64['_scale'][k]:.3e} ref {float(r64[k].norm()):.3e}")
    assert all(torch.isfinite(got[k]).all() for k in got)
    fam = c["fam"]
    n = c.get("N") if fam == "instnorm" else c.get("rows")
    if fam in ("instnorm", "bn") and n == 1:    # one term per statistic: dx and dgamma exactly zero (tests/train_cases.py has why)
        assert (got["dx"] == 0).all() and (got["dgamma"] == 0).all()
        if fam == "instnorm":                   # ... and y = fma(0 * rstd, gamma, beta) = beta, mean = x / 1
            assert torch.equal(got["y"], op["beta"].expand_as(got["y"])) and torch.equal(got["mean"], op["x"][:, 0])
    if c["kind"] == "const":                    # zero variance: xhat = 0 exactly, whatever the order of the sums
        ch = list(tc.const_channels(c["E"]))
        assert (got["dgamma"][ch] == 0).all()
        if fam == "instnorm":
            want = torch.tensor(tc.CONST_VALUES)
            assert torch.equal(got["mean"][:, ch], want.expand(c["B"], 3))
            assert torch.equal(got["y"][..., ch], op["beta"][ch].expand(c["B"], c["N"], 3))
    assert tc.misses(c, got, r64, r32) == []


@pytest.mark.parametrize("name", tc.NAMES)
def test_training_kernels_are_deterministic(name):
    """Two runs are bit-equal in every output -- fixed-order reductions -- except the instance norm's dgamma / dbeta over more than
    one instance: every workgroup adds its sums with float atomics, in an order that differs from run to run.  Those agree within
    the output's bound."""
    c = tc.CASES[name]
    op, r64, r32 = tc.reference(name)
    a, b = run_kernels(name), run_kernels(name)
    for k in tc.outputs(c):
        if c["fam"] == "instnorm" and k in ("dgamma", "dbeta") and c["B"] > 1:
            assert float((a[k].double() - b[k].double()).norm()) <= tc.bound(c, k, r64, r32)[1], k
        else:
            assert torch.equal(a[k], b[k]), k
