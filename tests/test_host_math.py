"""CPU: the case sets of tests/math_cases.py and the oracle's defined math on them.

tests/test_gpu_math.py holds every function of csrc/dmath.hpp to the oracle bit for bit on these sets, so the accuracies
measured here on the oracle are the device's as well.  Each bound below is the maximum MEASURED on the full set (against
float64 numpy, error in ulp of the float64 result rounded to float32), rounded up to the next quarter ulp (tanh: to the next
1e-8 absolute); both numbers stand side by side.  A bound that starts to fail means the oracle's arithmetic changed.

    function / set                                  measured max            bound
    d_expf  on [-87, 88]                            0.9956 ulp (8.392e-8)   1.0 ulp   smallest result 1.6458e-38 (normal)
    d_logf  on the noise domain (all 2^23 values)   0.8159 ulp, 4.907e-7    1.0 ulp
    d_logf  on [1, 2048]                            0.7583 ulp              1.0 ulp
    d_logf  around 2^e and sqrt(1/2) 2^e, all e     0.7484 ulp              0.75 ulp
    d_rcpf  on e^2a + 1 and around 2^e              0.5005 ulp (5.962e-8)   0.75 ulp  (94.9 % correctly rounded)
    d_tanhf on [-20, 20]                            7.448e-8 absolute       8e-8      never above 1 in magnitude
"""
import numpy as np
import pytest

import math_cases as mc


def ulp_err(got32, ref64):
    """|got - ref| in units of the spacing of float32 at the float64 reference rounded to float32."""
    r32 = ref64.astype(np.float32)
    return np.abs(got32.astype(np.float64) - ref64) / np.spacing(np.abs(r32)).astype(np.float64)


def is_normal_positive(bits):
    return (bits >= mc.FLT_MIN_BITS) & (bits <= mc.FLT_MAX_BITS)


def test_case_sets_have_the_stated_sizes_and_domains(oracle):
    e = mc.exp_bits()
    assert e.size % 4 == 0 and mc.exp_nonpos_bits().size % 4 == 0
    x = mc.b2f(mc.exp_nonpos_bits())
    with np.errstate(invalid="ignore"):
        assert ((x <= 0) | np.isnan(x)).all() and np.isnan(x).sum() >= 4 and (x == -np.inf).any()
    for special in (mc.f2b(-87.0), mc.f2b(-87.0) + 1, mc.f2b(88.0), 0, int(mc.SIGN), 1, mc.INF, mc.NINF, mc.QNAN, mc.FLT_MAX_BITS | int(mc.SIGN)):
        assert (e == special).any(), hex(special)
    # every tie (n + 1/2) ln 2 sits inside its +-64 ulp window: x log2 e (float32) rounds down on one side and up on the other
    for tie in mc.exp_tie_points()[::25]:
        t = mc.b2f(mc.around(tie)) * np.float32(1.44269504088896341)
        assert len(set(np.rint(t).tolist())) == 2
    lg = mc.log_bits()
    assert lg.size % 4 == 0 and is_normal_positive(lg).all(), "d_logf is defined for normal positive numbers"
    nd = mc.noise_domain_bits()
    assert nd.size == 1 << 23 and np.array_equal(lg[:nd.size], nd)
    u = mc.b2f(nd).astype(np.float64) * 2.0 ** 24
    assert np.array_equal(u, 2.0 * np.arange(1 << 23) + 1.0), "u = (2 k + 1) 2^-24 exactly"
    rc = mc.rcp_bits(lambda b: oracle.math_fn("exp", b))
    assert rc.size % 4 == 0 and is_normal_positive(rc).all(), "d_rcpf is defined for normal positive numbers"
    assert mc.tanh_bits().size % 4 == 0 and mc.noise_words().size % 4 == 0
    for s in (e, lg, mc.tanh_bits()):
        assert s.size <= 9_000_000
    v, perm, labels = mc.argmax_cases()
    assert sum(lb.startswith("pair") for lb in labels) == 2016 and v.shape == perm.shape == (len(labels), 64)
    zv, zi = mc.zrot_cases()
    assert {(int(a) & 3, int(b) & 3) for a, b in zi[:, :2]} == {(a, b) for a in range(4) for b in range(4)}
    assert sorted(set((zi[:, 1] - zi[:, 0]).tolist())) == list(range(1, 71))


def test_math_fn_agrees_with_the_existing_probe(oracle):
    x = np.concatenate([np.linspace(-87, 20, 5001), [1.0, 600.0, -0.0]]).astype(np.float32)
    e, l, t = oracle.math_probe(x)
    b = x.view(np.uint32)
    assert np.array_equal(oracle.math_fn("exp", b), e.view(np.uint32))
    assert np.array_equal(oracle.math_fn("tanh", b), t.view(np.uint32))
    pos = x > 0
    assert np.array_equal(oracle.math_fn("log", b[pos]), l[pos].view(np.uint32))


def test_exp_results_are_finite_normal_or_zero_and_accurate(oracle):
    b = mc.exp_bits()
    x = mc.b2f(b)
    e = mc.b2f(oracle.math_fn("exp", b))
    assert np.isfinite(e).all()
    assert ((e.view(np.uint32) == 0) | is_normal_positive(e.view(np.uint32))).all(), "exactly +0 or a normal positive number"
    with np.errstate(invalid="ignore"):
        dom = (x >= -87) & (x <= 88)
        below = ~(x >= -87)                          # x < -87, -inf and every NaN
    assert (e.view(np.uint32)[below] == 0).all(), "0 below -87, for -inf and for NaN"
    assert (e[x > 88] == e[x == 88][0]).all(), "clamped at 88"
    ref = np.exp(x[dom].astype(np.float64))
    err, rel = ulp_err(e[dom], ref).max(), (np.abs(e[dom] - ref) / ref).max()
    print(f"d_expf: {err:.4f} ulp, {rel:.4e} relative, smallest {e[dom].min():.5e}")
    assert err <= 1.0            # measured 0.9956
    assert rel <= 8.5e-8         # measured 8.392e-8 (1 ulp is at most 2^-23 = 1.19e-7 relative)


def test_log_accuracy(oracle):
    b = mc.log_bits()
    x = mc.b2f(b)
    got = mc.b2f(oracle.math_fn("log", b))
    ref = np.log(x.astype(np.float64))
    assert (got.view(np.uint32)[x == 1.0] == 0).all(), "log(1) is exactly +0"
    nz = ref != 0
    err = np.zeros_like(ref)
    err[nz] = ulp_err(got[nz], ref[nz])
    nd = 1 << 23
    n2 = nd + mc.stride(mc.f2b(1.0), mc.f2b(2048.0)).size
    absn = np.abs(got[:nd] - ref[:nd]).max()
    print(f"d_logf: noise {err[:nd].max():.4f} ulp {absn:.4e} abs; [1, 2048] {err[nd:n2].max():.4f} ulp; rest {err[n2:].max():.4f} ulp")
    assert err[:nd].max() <= 1.0 and absn <= 5e-7        # measured 0.8159 ulp, 4.907e-7
    assert err[nd:n2].max() <= 1.0                       # measured 0.7583
    assert err[n2:].max() <= 0.75                        # measured 0.7484


def test_rcp_accuracy(oracle):
    b = mc.rcp_bits(lambda bb: oracle.math_fn("exp", bb))
    x = mc.b2f(b)
    got = mc.b2f(oracle.math_fn("rcp", b))
    ref = 1.0 / x.astype(np.float64)
    err, rel = ulp_err(got, ref).max(), (np.abs(got - ref) / ref).max()
    print(f"d_rcpf: {err:.4f} ulp, {rel:.4e} relative, {np.mean(got == ref.astype(np.float32)):.4f} correctly rounded")
    assert err <= 0.75           # measured 0.5005: NOT always the correctly rounded quotient (0.5 ulp); dmath.hpp says so
    assert rel <= 6e-8           # measured 5.962e-8


def test_tanh_accuracy_and_specials(oracle):
    b = mc.tanh_bits()
    x = mc.b2f(b)
    got = mc.b2f(oracle.math_fn("tanh", b))
    fin = ~np.isnan(x)
    err = np.abs(got[fin] - np.tanh(x[fin].astype(np.float64))).max()
    print(f"d_tanhf: {err:.4e} absolute")
    assert err <= 8e-8           # measured 7.448e-8
    assert np.abs(got).max() == 1.0, "never above 1"
    assert np.array_equal(np.signbit(got), np.signbit(x)), "the sign is the argument's, for zeros and NaNs too"
    special = np.array([mc.QNAN, mc.QNAN_NEG, int(mc.SIGN), 0, mc.f2b(9.0), mc.INF, mc.NINF], np.uint32)
    want = np.array([0x3F800000, 0xBF800000, 0x80000000, 0, 0x3F7FFFFF, 0x3F800000, 0xBF800000], np.uint32)
    assert np.array_equal(oracle.math_fn("tanh", special), want)   # tanh(NaN) = 1, tanh(-0) = -0, tanh(9) = 0.99999994


def test_noise_words_map_to_exp1_draws(oracle):
    w = mc.noise_words()
    q = mc.b2f(oracle.math_fn("exp1_from_bits", w))
    u = ((2 * (w >> 9).astype(np.int64) + 1) * np.float32(2.0 ** -24)).astype(np.float32)
    assert np.array_equal(q.view(np.uint32), (np.float32(0) - mc.b2f(oracle.math_fn("log", u.view(np.uint32)))).view(np.uint32))
    assert (q > 0).all() and q[0] == q[2] and q[3] < q[2], "words 0 and 511 share u = 2^-24; 512 is the next u"
    assert np.abs(q + np.log(u.astype(np.float64))).max() <= 5e-7
    # the tensor entry point draws the same values from the same words
    R, T, M, seed = 3, 2, 7, 20261018
    ck = np.array([[qd, t, r, 0, seed & 0xFFFFFFFF, seed >> 32] for r in range(R) for t in range(T) for qd in range(2)], np.uint32)
    words = oracle.philox_words(ck).reshape(R, T, 8)[:, :, :M]
    assert np.array_equal(oracle.math_fn("exp1_from_bits", words).reshape(R, T, M), oracle.exp1_noise(seed, R, T, M).view(np.uint32))


def test_philox_oracle_equals_python_integers_and_the_known_answers(oracle):
    ck = mc.philox_cases()
    py = np.array([mc.philox4x32_10_python(r[:4], r[4:]) for r in ck], np.uint32)
    assert np.array_equal(oracle.philox_words(ck), py)
    assert py[:3].tolist() == mc.PHILOX_KAT


def test_wave_restatements(oracle):
    v = mc.wave_rows()
    tree = mc.ref_tree_sum(v)
    assert all(oracle.lane_tree(v[i]).view(np.uint32) == tree[i].view(np.uint32) for i in range(v.shape[0]))
    seq = np.zeros(v.shape[0], np.float32)
    for j in range(64):
        seq = seq + v[:, j]
    assert (seq != tree).sum() > 32, "the rows tell the tree order from a sequential sum"
    zv, zi = mc.zrot_cases()
    z = mc.ref_z_total(zv, zi)
    swapped = zi.copy()
    swapped[:, 0] += 1                      # the same weights taken as starting one node later: other pairs
    swapped[:, 1] += 1
    assert (mc.ref_z_total(zv, swapped) != z).mean() > 0.2, "the rows tell the pairing of an odd start from an even one"
    av, perm, labels = mc.argmax_cases()
    m, win = mc.ref_argmax(av, np.tile(np.arange(64, dtype=np.int32), (av.shape[0], 1)))
    assert np.array_equal(win, np.argmax(av, axis=1))
    k = labels.index("pair(3,60)")
    assert win[k] == 3 and mc.ref_argmax(av, perm)[1][k] == min(perm[k, 3], perm[k, 60])
    mv, mlabels = mc.max_rows()
    r = mc.ref_max(mv)
    assert np.isnan(r[mlabels.index("all NaN")]) and r[mlabels.index("NaN, finite lane 37")] == 2.5
    assert not np.isnan(r[mlabels.index("NaN in lane 5")])
