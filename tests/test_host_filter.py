"""Top-k / top-p filtering of a decode step, the part that needs no GPU: the test-side restatement (tests/filter_ref.py)
against the verdicts and log-probs recorded from the reference's own process_logits (tests/golden/filter_cases.npz,
make_golden_filter.py), and the C oracle's decode step, fed with synthetic caches (tests/filter_cases.py), against the same
recorded verdicts.

What catches which mistake (each tried by hand, in filter_ref.py for the first test and in oracle/eamrl_oracle.c for the second):
  `>=` for `>` in the top-k count (`<=` for `<` in the restatement) ... topk2_tie2, topk3_tie3, topk2_tie3_across64, masked_topk_tie, topk1_tie_at_top
  `<` for `<=` at the nucleus threshold ................................ uniform2_p0.5, uniform4_p0.5 / _p0.75, uniform5_p0.8, uniform128_p0.5, ...
  an unstable (here: descending-index) tie order ........................ uniform2_p0.5 (first), straddle_low_group, straddle_high_group, straddle_across64
  a normaliser taken from the first 64 entries only ..................... uniform128_p0.5 (first), straddle_across64, the random rows with M >= 65
  the threshold (float)(1 - (double)(float)top_p) ....................... uniform5_p0.8, uniform5_level3_p0.8, masked_low_high_uniform5, uniform10_p0.9
"""
import numpy as np

import filter_cases as fc
import filter_ref as fr
import make_golden_filter as mk

CASES = fc.load_cases()


def test_restatement_reproduces_every_recorded_verdict_and_logprob():
    crafted = [c for c in CASES if c["crafted"]]
    rand = [c for c in CASES if not c["crafted"]]
    # what the fixture holds
    assert [c["name"] for c in crafted] == [n for n, _, _, _ in mk.crafted()]
    for c, (_, a, k, p) in zip(crafted, mk.crafted()):
        assert np.array_equal(c["a"], a, equal_nan=True) and (c["top_k"], c["top_p"]) == (k, p)
        assert np.array_equal(c["x"], fc.crafted_x(a))
    for M in (2, 4, 5, 8, 10):
        for p in (0.5, 0.75, 0.8, 0.9):
            assert any(c["x"].size == M and c["top_p"] == p and c["top_k"] == 0 and (c["x"] == c["x"][0]).all() for c in crafted)
    combos = {(c["name"].split("_")[1], c["x"].size, c["top_p"], c["top_k"]) for c in rand}
    assert combos == {(f"s{s}", M, p, k) for s in fc.SCALES for M in fc.SIZES for p in fc.TOP_P for k in fc.top_ks(M)}
    assert all(0.01 <= c["top_p"] for c in rand)
    # the one row the old threshold formula decides differently: the reference removes one of five equally likely nodes
    five = next(c for c in crafted if c["name"] == "uniform5_p0.8")
    assert five["keep"].tolist() == [False, True, True, True, True]
    assert float(fr.threshold(0.8)) != float(np.float32(1.0 - np.float64(np.float32(0.8))))
    # the bound of the margin rule comes from the recorded rows
    observed = max(mk.noise_of(c["x"], c["top_k"]) for c in rand)
    assert observed == mk.OBSERVED and mk.MARGIN_BOUND == mk.MARGIN_FACTOR * observed
    skipped, worst = 0, 0.0
    for c in CASES:
        keep, logp, margin = fr.filter_row(c["x"], c["top_k"], c["top_p"])
        assert keep.any() and not np.isnan(c["logp"]).any()
        if c["crafted"]:
            fc.check_keep(c, keep, "restatement")
        elif margin < mk.MARGIN_BOUND:
            skipped += 1
            continue
        else:
            assert c["members"] and np.array_equal(keep, c["keep"]), (c["name"], margin)
        if c["members"]:
            assert np.array_equal(np.isfinite(logp), c["keep"])
            err = float(np.abs(c["logp"].astype(np.float64)[keep] - logp[keep]).max())
            assert err <= 1e-6, (c["name"], err)
            worst = max(worst, err)
        else:       # other members of a tie group: the same values at other places
            worst = max(worst, fc.check_logp(c["logp"], c["keep"], c["x"], 1e-6, c["name"]))
    print(f"crafted {len(crafted)}, random {len(rand)}, skipped by the margin rule {skipped} "
          f"({100.0 * skipped / len(rand):.2f} %), largest log-prob error {worst:.3g}")
    assert skipped <= fc.MAX_SKIP_SHARE * len(rand)


def _tsp_state(oracle, mask):
    B, M = mask.shape
    st = oracle.State("tsp", np.zeros((B, M, 2), np.float32))
    st.mask = np.ascontiguousarray(mask, dtype=np.uint8)
    return st


def test_oracle_decode_step_reproduces_the_recorded_keep_masks(oracle):
    for i, c in enumerate(CASES):
        if not c["crafted"]:
            continue
        cache, mask = fc.crafted_cache(c, i)
        st = _tsp_state(oracle, mask)
        act, lp, logits, logprobs = oracle.decode_step(st, cache, "greedy", clip=0.0, temp=1.0, num_heads=fc.H, want_all=True,
                                                       top_k=c["top_k"], top_p=c["top_p"])
        x = np.where(mask[0] != 0, logits[0], -np.inf).astype(np.float32)
        assert np.array_equal(x, c["x"]), (c["name"], "the synthetic cache does not give the recorded row")
        keep = np.isfinite(logprobs[0])
        fc.check_keep(c, keep, "oracle")
        fc.check_logp(logprobs[0], keep, x, 1e-5, c["name"])
        assert keep[act[0]] and lp[0] == logprobs[0, act[0]]
    rows = skipped = 0
    for M in fc.SIZES:
        cache, mask = fc.random_cache(M, 0)
        st = _tsp_state(oracle, mask)
        for p in fc.TOP_P:
            for k in fc.top_ks(M):
                act, lp, logits, logprobs = oracle.decode_step(st, cache, "greedy", clip=0.0, temp=1.0, num_heads=fc.H,
                                                               want_all=True, top_k=k, top_p=p)
                x = np.where(mask != 0, logits, -np.inf).astype(np.float32)
                for r in range(x.shape[0]):
                    rows += 1
                    keep, _, margin = fr.filter_row(x[r], k, p)
                    if margin < mk.MARGIN_BOUND:
                        skipped += 1
                        continue
                    got = np.isfinite(logprobs[r])
                    assert np.array_equal(got, keep), (M, p, k, r, margin, np.flatnonzero(got != keep).tolist())
                    fc.check_logp(logprobs[r], keep, x[r], 1e-5, (M, p, k, r))
                    assert keep[act[r]]
    print(f"random rows {rows}, skipped by the margin rule {skipped} ({100.0 * skipped / rows:.2f} %)")
    assert skipped <= fc.MAX_SKIP_SHARE * rows
