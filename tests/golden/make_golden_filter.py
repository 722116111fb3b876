#!/usr/bin/env python3
"""Fixture for the top-k / top-p filtering of a decode step, with verdicts recorded by RUNNING THE REFERENCE's own
`process_logits` (rl4co/utils/decoding.py:111-137,140-190; mask_logits=False, tanh_clipping=0, temperature=1) on the
CPU, one row at a time, in the build container:

    python tests/golden/make_golden_filter.py

Every case is a float32 row x (-inf where the env masked a node) with a top_k and a top_p; the reference's log-probs are
stored and its keep mask is where they are finite.  Nothing of the reference is copied, only what it returned.

Crafted cases sit on exact numbers: x = float32(a * float32(1 / sqrt(128))) for small integers a, which a decode step
reproduces bit for bit from a synthetic cache (tests/filter_cases.py).  Uniform rows of 2, 4, 5, 8, 10 (and 128, 256)
entries whose running sums land on the threshold; two and three entries tied at the k-th largest value; tie groups that
straddle the nucleus threshold, in the first 64 entries and across them; fewer, exactly as many and one finite entry
against top_k; -inf entries at low and high indices; the neutral settings top_k >= M, top_k = 1, top_p = 0 and 1; and
top_k with top_p where top-k removes the entries top-p would have counted.  Of a tie group the reference's sort (not
asked to be stable) may remove any members: `members` records per case whether it removed the ones an ascending stable
sort removes, i.e. whether the keep mask may be compared member by member; if not, only the number of members each tie
group lost is compared.  The restatement (tests/filter_ref.py) must reproduce every crafted verdict; none is skipped.

Random cases: logits N(0, s), s in {0.1, 1, 5}, M in {2, 5, 21, 64, 65, 101, 128, 129, 257}, top_p in {0.1, 0.5, 0.8,
0.95}, top_k in {0, 3, M // 2}, ROWS rows of each.  Two correct implementations that add the float32 running sum in
different orders (torch's CPU cumsum even accumulates in float64) may decide a row differently when a running sum comes
closer to the threshold than the rounding noise of such a sum.  That noise is measured on the data, not on any kernel:
the largest |float32 running sum - float64 running sum| over all recorded random rows is 5.010515451431274e-07 (eight ulp
of a sum just below 1; a row of 257 adds 256 roundings of up to half an ulp) -- OBSERVED below; MARGIN_FACTOR = 4 times
that is

    MARGIN_BOUND = 2.0042061805725098e-06

A random row whose `margin` (filter_ref.filter_row) is below MARGIN_BOUND takes no part in keep-set comparisons.  At most
1 % of the random rows may be skipped that way and no crafted row: asserted here and again by the tests.

top_p stays >= 0.01: below about 3e-8 the threshold float32(1 - top_p) rounds to 1.0, the last running sum (1.0, or a
last bit below) is then <= the threshold and the reference itself can remove every entry and return NaNs.  That is not
tested.

The archive is written with fixed time stamps, so a rerun gives the same bytes.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import filter_cases as fc  # noqa: E402
import filter_ref as fr  # noqa: E402
from make_golden_validity import write_npz  # noqa: E402

ROWS = 2                                  # random rows per (s, M, top_p, top_k)
MARGIN_FACTOR = 4
OBSERVED = 5.010515451431274e-07          # largest |cum32 - cum64| over the recorded random rows (asserted by main)
MARGIN_BOUND = MARGIN_FACTOR * OBSERVED
NAN = float("nan")


def crafted():
    """-> list of (name, a, top_k, top_p); a holds the column-0 values of Lp (nan = masked node)."""
    out = []
    for M in (2, 4, 5, 8, 10):
        for p in (0.5, 0.75, 0.8, 0.9):
            out.append((f"uniform{M}_p{p}", [0.0] * M, 0, p))
    out.append(("uniform5_level3_p0.8", [3.0] * 5, 0, 0.8))                  # the same at a non-zero logit
    out.append(("uniform128_p0.5", [0.0] * 128, 0, 0.5))                     # sum 64 / 128 == threshold: first block goes
    out.append(("uniform128_p0.75", [0.0] * 128, 0, 0.75))
    out.append(("uniform256_p0.5", [0.0] * 256, 0, 0.5))
    # ties at the k-th largest value (kept)
    out.append(("topk2_tie2", [5, 3, 3, 1, 0, 2], 2, 0.0))
    out.append(("topk3_tie3", [1, 4, 4, 4, 6, 0, 2, 7], 3, 0.0))
    a = [float(n % 7) for n in range(70)]
    a[3], a[64], a[69] = 9.0, 9.0, 9.0
    a[40] = 12.0
    out.append(("topk2_tie3_across64", a, 2, 0.0))                           # 12, then 9 three times (indices 3, 64, 69)
    # tie groups that straddle the nucleus threshold
    out.append(("straddle_low_group", [8, 0, 8, 0, 8, 0, 8, 0], 0, 0.8))     # two of the four low entries go
    out.append(("straddle_high_group", [8, 0, 8, 0, 8, 0, 8, 0], 0, 0.5))    # the low group and one high entry go
    out.append(("straddle_across64", [0.0] * 62 + [40.0] * 8, 0, 0.6))       # low group and entries 62, 63 of the high one
    # masked entries
    out.append(("fewer_finite_than_k", [3, NAN, 1, NAN, NAN, 2], 5, 0.0))
    out.append(("exactly_k_finite", [3, NAN, 1, NAN, NAN, 2], 3, 0.0))
    out.append(("fewer_finite_than_k_topp", [3, NAN, 1, NAN, NAN, 2], 5, 0.5))
    out.append(("one_finite_topk_topp", [NAN, NAN, 4, NAN], 2, 0.8))
    out.append(("one_finite_topp", [NAN, NAN, 4, NAN], 0, 0.9))
    out.append(("one_finite_topk1", [NAN, 4, NAN], 1, 0.0))
    out.append(("masked_low_high_uniform5", [NAN, 0, NAN, 0, 0, 0, 0, NAN], 0, 0.8))
    a = [0.0] * 70
    for n in (0, 5, 33, 34, 64, 69):
        a[n] = NAN
    out.append(("masked_low_high_uniform64_of_70", a, 0, 0.75))              # 64 finite: 16 / 64 == threshold
    out.append(("masked_topk_tie", [NAN, 5, 3, NAN, 3, 1, 3, NAN], 2, 0.0))
    # neutral settings
    out.append(("topk_eq_M", [2, 0, 1, 3], 4, 0.0))
    out.append(("topk_gt_M", [2, 0, 1, 3], 9, 0.0))
    out.append(("topk1", [2, 0, 5, 3], 1, 0.0))
    out.append(("topk1_tie_at_top", [5, 0, 5, 1], 1, 0.0))
    out.append(("topp0", [2, 0, 1, 3], 0, 0.0))
    out.append(("topp1", [2, 0, 1, 3], 0, 1.0))
    # top-k removes what top-p would have counted
    out.append(("topk_then_topp", [0, 0, 0, 0, 0, 0, 8, 8, 8, 8], 4, 0.5))   # top-p then halves the four that are left
    out.append(("topp_alone", [0, 0, 0, 0, 0, 0, 8, 8, 8, 8], 0, 0.5))       # ... alone it removes the six low ones only
    return [(n, np.asarray(a, np.float32), k, p) for n, a, k, p in out]


def random_cases():
    rng = np.random.default_rng(20261018)
    out = []
    for s in fc.SCALES:
        for M in fc.SIZES:
            for p in fc.TOP_P:
                for k in fc.top_ks(M):
                    for r in range(ROWS):
                        out.append((f"rand_s{s}_M{M}_p{p}_k{k}_{r}", (rng.standard_normal(M) * s).astype(np.float32), k, p))
    return out


def reference_logp(x, top_k, top_p):
    import _refshim

    _refshim.install()
    import torch
    from rl4co.utils.decoding import process_logits

    torch.set_num_threads(1)
    t = torch.from_numpy(x.copy())[None]
    out = process_logits(t, mask=None, temperature=1.0, top_p=top_p, top_k=top_k, tanh_clipping=0, mask_logits=False)
    return out[0].numpy().astype(np.float32)


def noise_of(x, top_k):
    """Largest |float32 running sum - float64 running sum| of the row after top-k."""
    x = x.copy()
    x[fr.top_k_removed(x, top_k)] = -np.inf
    _, _, c32, c64 = fr.running_sums(x)
    return float(np.abs(c32.astype(np.float64) - c64).max())


def main():
    cases = [(n, fc.crafted_x(a), a, k, p, True) for n, a, k, p in crafted()]
    cases += [(n, x, np.zeros_like(x), k, p, False) for n, x, k, p in random_cases()]
    rec = {k: [] for k in ("name", "crafted", "members", "top_k", "top_p", "x", "a", "keep", "logp")}
    skipped, nrand, observed, stable_differs = 0, 0, 0.0, []
    for name, x, a, k, p, is_crafted in cases:
        logp = reference_logp(x, k, p)
        assert not np.isnan(logp).any(), name
        keep = np.isfinite(logp)
        mine, mine_lp, margin = fr.filter_row(x, k, p)
        members = bool(np.array_equal(mine, keep))
        if is_crafted:
            assert fr.removed_per_group(x, mine) == fr.removed_per_group(x, keep), f"{name}: the restatement differs"
            if not members:
                stable_differs.append(name)
        else:
            nrand += 1
            observed = max(observed, noise_of(x, k))
            if margin < MARGIN_BOUND:
                skipped += 1
            else:
                assert members, f"{name}: the restatement differs from the reference at margin {margin:.3g}"
        for key, v in (("name", name), ("crafted", is_crafted), ("members", members), ("top_k", k), ("top_p", p), ("x", x),
                       ("a", a), ("keep", keep), ("logp", logp)):
            rec[key].append(v)
    assert observed == OBSERVED, f"OBSERVED in this file must read {observed!r}"
    assert skipped <= fc.MAX_SKIP_SHARE * nrand, (skipped, nrand)
    off = np.concatenate([[0], np.cumsum([x.size for x in rec["x"]])]).astype(np.int32)
    out = {"name": np.array(rec["name"]), "crafted": np.array(rec["crafted"]), "members": np.array(rec["members"]),
           "top_k": np.array(rec["top_k"], np.int32), "top_p": np.array(rec["top_p"], np.float64), "off": off,
           "x": np.concatenate(rec["x"]).astype(np.float32), "a": np.concatenate(rec["a"]).astype(np.float32),
           "keep": np.concatenate(rec["keep"]), "logp": np.concatenate(rec["logp"]).astype(np.float32)}
    write_npz(fc.PATH, out)
    print(f"filter_cases: {len(cases) - nrand} crafted, {nrand} random rows; skipped by the margin rule {skipped} "
          f"({100.0 * skipped / nrand:.2f} %); largest |cum32 - cum64| {observed!r}, bound {MARGIN_BOUND!r}; the reference's "
          f"sort left the stable order in {stable_differs}; {os.path.getsize(fc.PATH)} bytes", flush=True)


if __name__ == "__main__":
    main()
