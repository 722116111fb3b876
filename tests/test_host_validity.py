"""The solution-validity checks, the part that needs no GPU: the test-side restatement (tests/validity_ref.py) against the
verdicts recorded from the reference (tests/golden/validity_<env>.npz, make_golden_validity.py), what the fixtures hold,
the margin guarantee that makes exact comparison of verdicts fair, and the cases of tests/validity_cases.py that
test_gpu_validity.py builds on top of the fixtures (multistart layout, the wide CVRP graph)."""
import os
import re

import numpy as np
import pytest

import make_golden_validity as mk
import validity_ref as vr
from validity_cases import ENVS, expected_counters, fixture, multistart_case, top_id, wide_cvrp_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ENVS)
def test_restatement_reproduces_every_recorded_verdict(env):
    rows = 0
    for i, g in enumerate(fixture(env)):
        diff = np.flatnonzero(g["ref"].verdict != g["verdict"])
        assert diff.size == 0, (f"{env} group {i}: rows {diff[:8].tolist()} ({g['cls'][diff[:8]].tolist()}): restatement "
                                f"{g['ref'].verdict[diff[:8]].tolist()}, reference {g['verdict'][diff[:8]].tolist()}")
        assert set(np.unique(g["verdict"]).tolist()) <= {0, *vr.MESSAGE[env]}
        expected_counters(env, g)
        rows += g["verdict"].size
    print(env, "rows", rows)
    assert rows >= 100


@pytest.mark.parametrize("env", ENVS)
def test_fixtures_hold_every_class_and_enough_valid_rows(env):
    groups = fixture(env)
    labels = np.concatenate([g["cls"] for g in groups])
    verdict = np.concatenate([g["verdict"] for g in groups])
    for c in mk.CLASSES[env]:
        assert (labels == c).any(), f"{env}: no row of class {c}"
    assert set(labels.tolist()) <= set(mk.CLASSES[env])
    assert (verdict == 0).mean() >= 0.25
    # classes that are valid by name are valid, the others are not
    named_valid = np.array([c in ("valid", "wait_valid", "exact_full", "exact_at_limit", "exact_one", "exact_end") or c.endswith("_valid")
                            or c == "short_all_visited" for c in labels])
    assert np.array_equal(named_valid, verdict == 0)
    # shapes: node counts on both sides of 32, 64 and 128 and a wide one; row lengths on both sides of 64 and of 128
    tops = sorted(top_id(env, g) + (env == "tsp") for g in groups)
    assert tops == list(mk.NODES)
    T = [g["actions"].shape[1] for g in groups]
    assert min(T) < 64 and any(64 < t <= 128 for t in T) and max(T) > 128
    for g in groups:
        assert g["actions"].min() >= 0 and g["actions"].max() <= top_id(env, g)       # no ids out of range in the files
    # what the step- and id-specific classes claim
    for g in groups:
        for r in np.flatnonzero(np.char.startswith(g["cls"], "dup_id")):
            node = int(str(g["cls"][r])[6:])
            assert (g["actions"][r] == node).sum() != 1
        if env in ("cvrp", "cvrptw"):
            for r in np.flatnonzero(g["cls"] == "over_step64"):
                a = g["actions"][r]
                raw = np.round(g["demand"][g["inst"][r]].astype(np.float64) * 1920).astype(np.int64)   # 1920 = lcm(30, 64)
                assert mk.first_over_step(a.tolist(), raw, 1920) >= 64


@pytest.mark.parametrize("env", ENVS)
def test_margin_guarantee_holds_for_the_committed_fixtures(env):
    exact = 0
    for g in fixture(env):
        mk.check_margins(env, g, g["ref"])
        exact += int(g["exact"].sum())
        assert np.array_equal(g["exact"], g["ref"].margin < mk.MARGIN)
    print(env, "rows decided on exactly representable numbers:", exact)
    if env == "op":
        assert exact == 0                  # a sum of square roots is never exact: every row keeps its distance
    if env in ("cvrp", "pctsp"):
        assert exact > 0                   # load == capacity, prize == 1


def test_exact_edge_rows_sit_on_their_thresholds():
    for g in fixture("cvrp"):
        for r in np.flatnonzero(np.isin(g["cls"], ("exact_full", "exact_over"))):
            raw = np.round(g["demand"][g["inst"][r]].astype(np.float64) * 64).astype(np.int64)
            load, peak = 0, 0
            for a in g["actions"][r]:
                load = 0 if a == 0 else load + int(raw[a - 1])
                peak = max(peak, load)
            assert peak == (64 if g["cls"][r] == "exact_full" else 65)
    # the capacity limit itself: float32(1 + 1e-5) = 1 + 84 * 2^-23 is reached exactly (valid) or passed by one ulp, at
    # step 1, at a step >= 64 and in the last route.  `>=` in place of `>` flips every exact_at_limit row.
    lim = np.float32(1.0) + np.float32(1e-5)
    assert float(lim) == 1.0 + 84 * mk.ULP
    where = {"exact_at_limit": set(), "exact_ulp_over": set()}
    for g in fixture("cvrp"):
        for r in np.flatnonzero(np.isin(g["cls"], tuple(where))):
            dem = np.concatenate([[0.0], g["demand"][g["inst"][r]].astype(np.float64)])
            a = g["actions"][r]
            assert g["capacity"][g["inst"][r]] == 1.0
            load, peak, step = 0.0, 0.0, None
            for t, x in enumerate(a):
                load = max(0.0, load - 1.0) if x == 0 else load + dem[x]       # exact in float64: multiples of 2^-23 below 4
                if load > peak:
                    peak, step = load, t
            assert peak == float(lim) + (mk.ULP if g["cls"][r] == "exact_ulp_over" else 0.0)
            assert g["verdict"][r] == (vr.OVER_CAPACITY if g["cls"][r] == "exact_ulp_over" else 0)
            where[str(g["cls"][r])] |= {"step1"} if step == 1 else set()
            where[str(g["cls"][r])] |= {"step64"} if step >= 64 else set()
            where[str(g["cls"][r])] |= {"last"} if (a[step + 1:] == 0).all() else set()
    assert where == {"exact_at_limit": {"step1", "step64", "last"}, "exact_ulp_over": {"step1", "step64", "last"}}
    for g in fixture("pctsp"):
        for r in np.flatnonzero(np.isin(g["cls"], ("exact_one", "exact_short"))):
            a = g["actions"][r]
            total = float(g["real_prize"][g["inst"][r]].astype(np.float64)[a].sum())
            assert total == (1.0 if g["cls"][r] == "exact_one" else 63 / 64) and (a != 0).sum() < top_id("pctsp", g)
    for g in fixture("cvrptw"):
        for r in np.flatnonzero(np.isin(g["cls"], ("exact_end", "exact_one_late"))):
            b = g["inst"][r]
            locs, tw, dur = g["locs"][b].astype(np.int64), g["time_windows"][b], g["durations"][b]
            clock, node, at_end, one_late = 0, 0, 0, 0
            n = min(12, top_id("cvrptw", g))
            for a in g["actions"][r][:n]:                  # the first legs are 3-4-5 triangles: integer arithmetic
                d2 = int(((locs[node] - locs[a]) ** 2).sum())
                leg = int(round(d2 ** 0.5))
                assert leg * leg == d2 and a != 0
                start = max(clock + leg, int(tw[a, 0]))
                at_end += start == tw[a, 1]
                one_late += start == tw[a, 1] + 1
                clock, node = start + int(dur[a]), a
            assert (at_end, one_late) == (n, 0) if g["cls"][r] == "exact_end" else one_late == 1
            assert g["verdict"][r] == (0 if g["cls"][r] == "exact_end" else vr.LATE)
        late = np.flatnonzero(g["cls"] == "exact_one_late")
        assert late.size >= 1


@pytest.mark.parametrize("env", ENVS[1:])
@pytest.mark.parametrize("S", [3, 5])
def test_multistart_cases_tell_the_row_mapping_apart(env, S):
    sub, actions, right, wrong = multistart_case(env, S)
    B = 3
    assert actions.shape[0] == S * B
    own = np.arange(S * B) // B % 2 == 0
    assert (right.verdict[own] == 0).all(), "a tour is valid for its own instance"
    assert (right.verdict[~own] != 0).any(), "a neighbour's tour is invalid here"
    assert not np.array_equal(right.counters.sum(0), wrong.counters.sum(0)), "the wrong mapping gives other counts"
    for r in range(S * B):                 # the margin guarantee for the rows that are judged by another instance
        assert right.margin[r] >= mk.MARGIN or mk.representable(env, sub, r % B), (env, r, right.margin[r])


def test_wide_cvrp_case():
    demand, cap, actions = wide_cvrp_case()
    res = vr.cvrp(demand, cap, actions)
    assert res.verdict.tolist() == [0, vr.INVALID_TOUR, vr.INVALID_TOUR, vr.OVER_CAPACITY]
    assert 1090 <= actions.shape[1] <= 1200


def test_out_of_range_ids_are_invalid_tours_in_the_restatement():
    for env in ENVS:
        g = fixture(env)[3]
        r = int(np.flatnonzero(g["verdict"] == 0)[0])
        for bad in (-1, top_id(env, g) + 1, 2 ** 40):
            a = g["actions"][r:r + 1].copy()
            a[0, 1] = bad
            res = mk.evaluate(env, g, actions=a, inst=g["inst"][r:r + 1])
            assert res.verdict.tolist() == [vr.RANGE] and res.counters[0, 0] == 1 and res.counters[0, 1] == 0


def test_messages_are_the_ones_the_envs_raise():
    """The messages of an env's two counters are stated once, in env_spec, in the order of the counters; the env classes
    assert with exactly those.  The time-window message is the env class's own."""
    from eam_rl4co_amd import envs
    from eam_rl4co_amd.env_spec import spec

    with open(os.path.join(ROOT, "eam_rl4co_amd", "envs.py")) as f:
        text = f.read()
    for env in ENVS:
        own = spec(envs.ENV_REGISTRY[env].name).messages
        for code, msg in vr.MESSAGE[env].items():
            if code == vr.LATE:
                assert re.search(re.escape(f'"{msg}'), text), msg
            else:
                assert msg in own, msg
    # no second copy of a counter message in the env classes
    for msg in {m for env in ENVS for m in spec(env).messages}:
        assert f'"{msg}' not in text, msg
