"""Input sets for the defined math of csrc/dmath.hpp, as BIT PATTERNS (uint32), shared by tests/test_host_math.py (CPU) and
tests/test_gpu_math.py (GPU).  Pure numpy.  Every elementwise set is padded to a multiple of 4 (the four slots of a wide call)
by repeating its first element; the sets are built once per process and returned read-only.

"Every 257th pattern of [a, b]" means the bit patterns bits(a), bits(a) + 257, ... <= bits(b) of one sign: 257 is odd, so the
low mantissa bits run through all their values.  "+-64 ulp around x" means the 129 patterns bits(x) - 64 .. bits(x) + 64.

exp_bits()            d_expf and its five wide forms
    every 257th pattern from 1 up to 88.0 and, with the sign bit, up to -87.0 (8,706,344 values; on these the wide forms'
    add-magic rounding must equal rint and their shifted scale (n + 127) << 23);
    +-64 ulp around -87, 88, +0, -0 (these are denormals) and around every rounding tie (n + 1/2) ln 2, n = -126 .. 127;
    -87 and its predecessor; denormals of both signs at every 2^16th pattern, the smallest and the largest;
    every 65537th pattern from -87 down to -FLT_MAX and from 88 up to FLT_MAX (beyond |x log2 e| >= 2^22 the magic rounding is
    no longer exact: only the final select keeps the result), +-64 ulp around -+2^22 ln 2 and below FLT_MAX of both signs;
    -inf, +inf, quiet NaNs of both signs, a NaN with a payload, a signalling NaN.
exp_nonpos_bits()     the subset x <= 0 (both zeros) of the above plus every NaN: the domain of the _nonpos forms.
log_bits()            d_logf, d_logf4
    ALL 2^23 values u = (2 k + 1) 2^-24: the whole domain of the sampling noise;
    every 257th pattern of [1, 2048] (softmax denominators of up to 2048 terms <= 1);
    +-64 ulp around 2^e and around sqrt(1/2) 2^e (the m < sqrt(1/2) branch) for every normal exponent e = -126 .. 127, clipped
    to the normal numbers; FLT_MIN and FLT_MAX.
tanh_bits()           d_tanhf, d_tanhf2, d_tanhf4
    every 257th pattern of [0, 20], both signs; +-64 ulp around +-0.625 and +-9.0 (the two switches); +-0, +-inf, the NaNs,
    the denormals of exp_bits().
rcp_bits(exp_fn)      d_rcpf: e + 1 for e = d_expf(a + a), a over every 257th pattern of [0.625, 9] (what d_tanhf feeds it; exp_fn
    maps bit patterns to d_expf's bit patterns); +-64 ulp around 2^e, e = -125 .. 125 (x and 1 / x both normal numbers).
noise_words()         exp1_from_bits: 0, 0xFFFFFFFF, 511, 512 (the >> 9 boundary) and 2^16 random words.
philox_cases()        [G, 6] counter / key words: all zero, all ones, the Random123 "pi" vector, counters as the noise uses them
    (node quad, step, row low, row high) with 64-bit seeds, random words.

Wave sets are [W, 64] rows, one wavefront each (wave_rows(), argmax_cases(), max_rows(), zrot_cases()); see each function.
"""
from __future__ import annotations

import functools

import numpy as np

SIGN = np.uint32(0x80000000)
QNAN, QNAN_NEG, NAN_PAYLOAD, SNAN = 0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7F800001
NANS = np.array([QNAN, QNAN_NEG, NAN_PAYLOAD, SNAN], np.uint32)
INF, NINF = 0x7F800000, 0xFF800000
FLT_MIN_BITS, FLT_MAX_BITS = 0x00800000, 0x7F7FFFFF


def f2b(x) -> int:
    return int(np.array(x, np.float32).view(np.uint32))


def b2f(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def stride(lo_bits: int, hi_bits: int, step: int = 257, neg: bool = False):
    """lo_bits, lo_bits + step, ... <= hi_bits (magnitudes), with the sign bit if neg."""
    a = np.arange(lo_bits, hi_bits + 1, step, dtype=np.uint32)
    return a | SIGN if neg else a


def around(x, k: int = 64):
    """the 2 k + 1 patterns bits(x) - k .. bits(x) + k (x != 0, same sign throughout)."""
    b = f2b(x)
    assert (b & 0x7FFFFFFF) > k
    return np.arange(b - k, b + k + 1, dtype=np.uint32)


def _finish(parts):
    a = np.concatenate([np.asarray(p, np.uint32).ravel() for p in parts])
    pad = (-a.size) % 4
    if pad:
        a = np.concatenate([a, np.repeat(a[:1], pad)])
    a.setflags(write=False)
    return a


def denormal_bits():
    d = np.concatenate([np.arange(1, 65, dtype=np.uint32), np.arange(1, FLT_MIN_BITS, 1 << 16, dtype=np.uint32),
                        np.array([FLT_MIN_BITS - 1], np.uint32)])
    return np.concatenate([d, d | SIGN])


def exp_tie_points():
    """float32 nearest to (n + 1/2) ln 2, n = -126 .. 127: where rint(x log2 e) changes."""
    n = np.arange(-126, 128, dtype=np.float64)
    return ((n + 0.5) * np.log(2.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def exp_bits():
    parts = [stride(1, f2b(88.0)), stride(1, f2b(87.0), neg=True)]
    assert parts[0].size + parts[1].size == 8706344
    parts += [around(-87.0), around(88.0), np.arange(0, 65, dtype=np.uint32), np.arange(0, 65, dtype=np.uint32) | SIGN]
    parts += [around(x) for x in exp_tie_points()]
    parts += [[f2b(-87.0), f2b(-87.0) + 1], denormal_bits()]
    parts += [stride(f2b(87.0), FLT_MAX_BITS, 65537, neg=True), stride(f2b(88.0), FLT_MAX_BITS, 65537)]
    big = np.float32(2.0 ** 22 * np.log(2.0))
    parts += [around(big), around(-big), np.arange(FLT_MAX_BITS - 64, FLT_MAX_BITS + 1, dtype=np.uint32),
              np.arange(FLT_MAX_BITS - 64, FLT_MAX_BITS + 1, dtype=np.uint32) | SIGN]
    parts += [[NINF, INF], NANS]
    return _finish(parts)


@functools.lru_cache(maxsize=None)
def exp_nonpos_bits():
    b = exp_bits()
    x = b2f(b)
    with np.errstate(invalid="ignore"):
        keep = (x <= 0) | np.isnan(x)
    return _finish([b[keep]])


@functools.lru_cache(maxsize=None)
def noise_domain_bits():
    """all u = (2 k + 1) 2^-24, k = 0 .. 2^23 - 1 (exact in float32)."""
    u = (2.0 * np.arange(1 << 23, dtype=np.float32) + 1.0) * np.float32(2.0 ** -24)
    return u.view(np.uint32)


@functools.lru_cache(maxsize=None)
def log_bits():
    parts = [noise_domain_bits(), stride(f2b(1.0), f2b(2048.0))]
    for e in range(-126, 128):
        for x in (np.float32(2.0 ** e), np.float32(np.sqrt(0.5) * 2.0 ** e)):
            parts.append(np.clip(around(x).astype(np.int64), FLT_MIN_BITS, FLT_MAX_BITS).astype(np.uint32))
    parts.append([FLT_MIN_BITS, FLT_MAX_BITS])
    return _finish(parts)


@functools.lru_cache(maxsize=None)
def tanh_bits():
    parts = [stride(0, f2b(20.0)), stride(0, f2b(20.0), neg=True)]
    parts += [around(0.625), around(-0.625), around(9.0), around(-9.0)]
    parts += [[0, int(SIGN), INF, NINF], NANS, denormal_bits()]
    return _finish(parts)


def rcp_bits(exp_fn):
    a = b2f(stride(f2b(0.625), f2b(9.0)))
    e = b2f(exp_fn((a + a).view(np.uint32)))
    parts = [(e + np.float32(1.0)).view(np.uint32)]
    parts += [around(np.float32(2.0 ** e)) for e in range(-125, 126)]
    return _finish(parts)


@functools.lru_cache(maxsize=None)
def noise_words():
    rng = np.random.default_rng(20261018)
    return _finish([[0, 0xFFFFFFFF, 511, 512], rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)])


@functools.lru_cache(maxsize=None)
def philox_cases():
    rng = np.random.default_rng(4)
    rows = [[0] * 6, [0xFFFFFFFF] * 6,
            [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0]]
    for quad, step, row, seed in ((0, 0, 0, 7), (24, 99, 102399, 20261018), (255, 1023, (1 << 33) + 5, 0xFEDCBA9876543210)):
        rows.append([quad, step, row & 0xFFFFFFFF, row >> 32, seed & 0xFFFFFFFF, seed >> 32])
    ck = np.concatenate([np.array(rows, np.uint64), rng.integers(0, 1 << 32, (250, 6), dtype=np.uint64)]).astype(np.uint32)
    ck.setflags(write=False)
    return ck


def philox4x32_10_python(c, k):
    """Philox4x32-10 in Python integers (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped by the Weyl constants
    between rounds.  A third statement beside the device's and the oracle's, sharing no code with either."""
    m0, m1, w0, w1, mask = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c0, c1, c2, c3 = (int(x) for x in c)
    k0, k1 = (int(x) for x in k)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & mask, (p0 >> 32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + w0) & mask, (k1 + w1) & mask
    return [c0, c1, c2, c3]


# Random123's known-answer vectors for philox4x32 with 10 rounds (counter, key -> words): rows 0 .. 2 of philox_cases()
PHILOX_KAT = [
    [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8],
    [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD],
    [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1],
]


# ---------------------------------------------------------------------------------------------------------------------
# wave sets: [W, 64] float32 rows (returned as float32; view them as uint32 to pass them on)
# ---------------------------------------------------------------------------------------------------------------------
def spread_rows(rng, n):
    """magnitudes spread over 2^-20 .. 2^20, both signs: a different summation order changes the bits of the sum."""
    return (rng.uniform(0.5, 1.0, (n, 64)) * np.exp2(rng.integers(-20, 21, (n, 64))) * rng.choice([-1.0, 1.0], (n, 64))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def wave_rows():
    """64 standard-normal rows, then 64 spread rows."""
    rng = np.random.default_rng(11)
    v = np.concatenate([rng.standard_normal((64, 64)).astype(np.float32), spread_rows(rng, 64)])
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def argmax_cases():
    """(v [W, 64] float32, perm [W, 64] int32, label list).  Every pair of lanes i < j holding the same maximum (2016 cases,
    the other lanes random below it); all lanes equal; all -inf; one finite lane among -inf at every position (64); 64 rows of
    values from {0, 1, 2} (many ties at every butterfly level).  perm is a per-case permutation of 0 .. 63 with the
    offset 1000 (an index that is not the lane number)."""
    rng = np.random.default_rng(12)
    rows, labels = [], []
    for i in range(64):
        for j in range(i + 1, 64):
            r = rng.uniform(-1.0, 1.0, 64).astype(np.float32)
            r[i] = r[j] = np.float32(1.5)
            rows.append(r)
            labels.append(f"pair({i},{j})")
    rows.append(np.full(64, 0.25, np.float32)); labels.append("all equal")
    rows.append(np.full(64, -np.inf, np.float32)); labels.append("all -inf")
    for i in range(64):
        r = np.full(64, -np.inf, np.float32)
        r[i] = np.float32(-3.0)
        rows.append(r)
        labels.append(f"finite lane {i} among -inf")
    for k in range(64):
        rows.append(rng.integers(0, 3, 64).astype(np.float32))
        labels.append(f"ties {k}")
    v = np.stack(rows)
    perm = np.stack([rng.permutation(64) for _ in range(v.shape[0])]).astype(np.int32) + 1000
    v.setflags(write=False)
    perm.setflags(write=False)
    return v, perm, labels


@functools.lru_cache(maxsize=None)
def max_rows():
    """(v [W, 64] float32, labels): the 128 rows of wave_rows(); a quiet NaN in lane p alone for every p (64 rows, the rest
    random); NaN in all lanes; all -inf; -inf with one finite lane (lanes 0, 31, 63); NaN everywhere but one lane (0, 37)."""
    rng = np.random.default_rng(13)
    rows, labels = list(wave_rows()), [f"row {i}" for i in range(128)]
    nan = b2f(np.array([QNAN], np.uint32))[0]
    for p in range(64):
        r = rng.standard_normal(64).astype(np.float32)
        r[p] = nan
        rows.append(r); labels.append(f"NaN in lane {p}")
    rows.append(np.full(64, nan, np.float32)); labels.append("all NaN")
    rows.append(np.full(64, -np.inf, np.float32)); labels.append("all -inf")
    for p in (0, 31, 63):
        r = np.full(64, -np.inf, np.float32); r[p] = np.float32(-7.5)
        rows.append(r); labels.append(f"-inf, finite lane {p}")
    for p in (0, 37):
        r = np.full(64, nan, np.float32); r[p] = np.float32(2.5)
        rows.append(r); labels.append(f"NaN, finite lane {p}")
    v = np.stack(rows)
    v.setflags(write=False)
    return v, labels


@functools.lru_cache(maxsize=None)
def zrot_cases():
    """(v [280, 64] float32 spread rows, idx [280, 64] int32 with idx[:, 0] = start, idx[:, 1] = n1 = start + length) for the
    lengths 1 .. 70 crossed with start = 0 .. 3 (so start and n1 take every residue mod 4)."""
    rng = np.random.default_rng(14)
    v = spread_rows(rng, 280)
    idx = np.zeros((280, 64), np.int32)
    k = 0
    for length in range(1, 71):
        for start in range(4):
            idx[k, 0], idx[k, 1] = start, start + length
            k += 1
    v.setflags(write=False)
    idx.setflags(write=False)
    return v, idx


# ---------------------------------------------------------------------------------------------------------------------
# plain restatements of the wavefront primitives (float32 numpy)
# ---------------------------------------------------------------------------------------------------------------------
def ref_tree_sum(v):
    """adjacent pairs, six times -> [W] float32."""
    v = np.asarray(v, np.float32)
    for _ in range(6):
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def ref_max(v):
    """max with NaNs ignored (NaN only if all are) -> [W]."""
    return np.fmax.reduce(np.asarray(v, np.float32), axis=1)


def ref_vmax(v, k):
    """lane l: max of v[(l + 0) % 64] .. v[(l + k - 1) % 64], NaNs ignored -> [W, 64]."""
    v = np.asarray(v, np.float32)
    out = v.copy()
    for s in range(1, k):
        out = np.fmax(out, np.roll(v, -s, axis=1))
    return out


def ref_argmax(v, idx):
    """(max, the smallest idx among its holders) per row."""
    v = np.asarray(v, np.float32)
    m = v.max(axis=1)
    big = np.iinfo(np.int64).max
    win = np.where(v == m[:, None], idx.astype(np.int64), big).min(axis=1)
    return m, win.astype(np.int32)


def ref_z_total(v, idx):
    """canonical softmax-denominator order for every lane: node n = start .. n1 - 1 of lane l weighs v[(l + n - start) % 64];
    P_r = sequential float32 sum (from +0) of the nodes n = r (mod 4), ascending; (P0 + P1) + (P2 + P3) -> [W, 64]."""
    v = np.asarray(v, np.float32)
    W = v.shape[0]
    out = np.empty((W, 64), np.float32)
    for w in range(W):
        start, n1 = int(idx[w, 0]), int(idx[w, 1])
        P = [np.zeros(64, np.float32) for _ in range(4)]
        for n in range(start, n1):
            P[n & 3] = P[n & 3] + np.roll(v[w], -(n - start))      # one float32 add per lane, in node order
        out[w] = (P[0] + P[1]) + (P[2] + P[3])
    return out
