"""GPU: every function of csrc/dmath.hpp, called one by one through the probes of csrc/math_probe.hip, against the CPU oracle
(exp, log, rcp, tanh, the noise transform, Philox) and against the numpy restatements of tests/math_cases.py (the wavefront
primitives).  Everything is compared BIT FOR BIT (uint32 views; no +0 / -0 or NaN leniency), on the sets that
tests/math_cases.py states: the clamps at -87 / 88, every rounding tie of the add-magic rint, the sqrt(1/2) branch of the
log, the 0.625 / 9.0 switches of tanh, NaN / inf / denormals, every pair of lanes that can tie in the argmax butterfly, every
start / end residue of the rotating softmax denominators.

Each wide form gets the input array rotated by 0 .. 3 elements, so that every input passes through every slot of the form.
The comparison runs on the device; only mismatches travel back.  What is pinned is the header's function as the library's
flags compile it in the probe's translation unit, not each inlined copy in the kernels that include the header (those are
held to the oracle through whole rollouts, tests/test_gpu_parity.py).
"""
import numpy as np
import pytest
import torch

import math_cases as mc
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu


def dev(bits):
    return torch.from_numpy(np.array(bits, copy=True).view(np.int32)).to(DEV)      # the sets are read-only: upload a copy


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def mismatches(fn, x_bits, want_bits, rotations):
    """list of messages naming the first inputs at which ops.math_probe(fn) differs from want, over the rotations."""
    from eam_rl4co_amd import ops

    x, want = dev(x_bits), dev(want_bits)
    out = []
    for rot in rotations:
        xr, wr = torch.roll(x, rot), torch.roll(want, rot)
        got = ops.math_probe(fn, xr)
        if not torch.equal(got, wr):
            bad = (got != wr).nonzero().flatten()
            i = bad[:4]
            rows = [f"x={a:08x} got={g:08x} want={w:08x} slot={int(k) % 4}"
                    for a, g, w, k in zip(u32(xr[i]), u32(got[i]), u32(wr[i]), i.cpu())]
            out.append(f"{fn} rot {rot}: {bad.numel()} of {x.numel()} differ: " + "; ".join(rows))
    return out


def check(forms, x_bits, want_bits):
    """forms: {probe name: width}; a form of width w is run with the rotations 0 .. 3 (scalar forms once)."""
    bad = []
    for fn, width in forms.items():
        bad += mismatches(fn, x_bits, want_bits, range(4) if width > 1 else (0,))
    assert not bad, "\n".join(bad)


def test_exp_forms_equal_the_oracle(oracle):
    b = mc.exp_bits()
    check({"expf": 1, "expf2": 2, "expf4": 4}, b, oracle.math_fn("exp", b))


def test_exp_nonpos_forms_equal_the_oracle(oracle):
    """x <= 0 and NaN: no lower clamp in these forms, the final select alone makes the exact +0 below -87."""
    b = mc.exp_nonpos_bits()
    want = oracle.math_fn("exp", b)
    x = mc.b2f(b)
    with np.errstate(invalid="ignore"):
        assert (want[~(x >= -87)] == 0).all()           # -inf, NaN, everything below -87: the oracle's +0
    check({"expf2_nonpos": 2, "expf2_nonpos_x2": 4, "expf4_nonpos": 4}, b, want)


def test_log_forms_equal_the_oracle(oracle):
    b = mc.log_bits()
    check({"logf": 1, "logf4": 4}, b, oracle.math_fn("log", b))


def test_rcp_equals_the_oracle(oracle):
    b = mc.rcp_bits(lambda bb: oracle.math_fn("exp", bb))
    check({"rcpf": 1}, b, oracle.math_fn("rcp", b))


def test_tanh_forms_equal_the_oracle(oracle):
    """NaN, inf, -0 included: whatever the oracle returns (tanh(NaN) = 1, tanh(-0) = -0, tanh(9) = 0.99999994)."""
    b = mc.tanh_bits()
    want = oracle.math_fn("tanh", b)
    special = {mc.QNAN: 0x3F800000, int(mc.SIGN): 0x80000000, mc.f2b(9.0): 0x3F7FFFFF}
    for k, v in special.items():
        assert (want[b == k] == v).all() and (b == k).any()
    check({"tanhf": 1, "tanhf2": 2, "tanhf4": 4}, b, want)


def test_noise_transform_equals_the_oracle(oracle):
    w = mc.noise_words()
    u = ((2 * (w >> 9).astype(np.int64) + 1) * 2.0 ** -24).astype(np.float32)
    want = (np.float32(0) - mc.b2f(oracle.math_fn("log", u.view(np.uint32)))).view(np.uint32)
    assert np.array_equal(want, oracle.math_fn("exp1_from_bits", w))
    check({"exp1_from_bits": 1}, w, want)


def test_philox_words_equal_the_oracle_and_python_integers(oracle):
    from eam_rl4co_amd import ops

    ck = mc.philox_cases()
    got = u32(ops.math_probe("philox", dev(ck)))
    py = np.array([mc.philox4x32_10_python(r[:4], r[4:]) for r in ck], np.uint32)
    assert np.array_equal(got, oracle.philox_words(ck)), "device words != oracle words"
    assert np.array_equal(got, py), "device words != the Python-integer restatement"
    assert got[:3].tolist() == mc.PHILOX_KAT, "Random123 known answers"


def assert_all_lanes(got, want, labels, what):
    """got [W, 64] uint32 against want [W] or [W, 64] uint32: every lane of every case."""
    want = np.broadcast_to(want[:, None] if want.ndim == 1 else want, got.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} lanes differ; first: " + "; ".join(
        f"case {labels[w] if labels else w} lane {l}: got {got[w, l]:08x} want {want[w, l]:08x}" for w, l in bad[:4])


def test_wave_tree_sum_is_the_adjacent_pair_tree():
    from eam_rl4co_amd import ops

    v = mc.wave_rows()
    got = u32(ops.wave_probe("tree_sum", dev(v.view(np.uint32))))
    assert_all_lanes(got, mc.ref_tree_sum(v).view(np.uint32), None, "wave_tree_sum")


def test_max_forms_ignore_nans_in_every_lane():
    from eam_rl4co_amd import ops

    v, labels = mc.max_rows()
    vb = dev(v.view(np.uint32))
    assert_all_lanes(u32(ops.wave_probe("max", vb)), mc.ref_max(v).view(np.uint32), labels, "wave_max")
    for fn, k in (("vmax", 2), ("vmax3", 3), ("vmax5", 5)):
        assert_all_lanes(u32(ops.wave_probe(fn, vb)), mc.ref_vmax(v, k).view(np.uint32), labels, fn + "_raw")


def test_wave_argmax_takes_the_lowest_index_in_all_lanes():
    from eam_rl4co_amd import ops

    v, perm, labels = mc.argmax_cases()
    vb = dev(v.view(np.uint32))
    lane = np.tile(np.arange(64, dtype=np.int32), (v.shape[0], 1))
    for idx, what in ((lane, "idx = lane"), (perm, "permuted idx")):
        m, win = mc.ref_argmax(v, idx)
        got_v, got_i = ops.wave_probe("argmax", vb, dev(idx))
        assert_all_lanes(u32(got_i), win.view(np.uint32), labels, f"wave_argmax index, {what}")
        assert_all_lanes(u32(got_v), m.view(np.uint32), labels, f"wave_argmax value, {what}")


def test_rotating_denominators_follow_the_canonical_order():
    from eam_rl4co_amd import ops

    v, idx = mc.zrot_cases()
    want = mc.ref_z_total(v, idx).view(np.uint32)
    labels = [f"start {a} n1 {b}" for a, b in idx[:, :2]]
    vb, ib = dev(v.view(np.uint32)), dev(idx)
    assert_all_lanes(u32(ops.wave_probe("zrot", vb, ib)), want, labels, "ZRot::total")
    assert_all_lanes(u32(ops.wave_probe("z_total_rel", vb, ib)), want, labels, "z_total_rel")
