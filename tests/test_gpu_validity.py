"""The solution-validity kernels (eamrl_check_solution for TSP / CVRP / SDVRP / PCTSP, eamrl_op_check_solution,
eamrl_cvrptw_check_time, and the second TSP / CVRP copy inside eamrl_rollout_finish) against the verdicts recorded from the
reference (tests/golden/validity_<env>.npz; tests/validity_ref.py is pinned to them by test_host_validity.py).  Verdicts
and counts are compared exactly; the fixtures guarantee that no row depends on the order of a float32 sum."""
import numpy as np
import pytest
import torch

import make_golden_validity as mk
import validity_ref as vr
from test_gpu_parity import DEV, t
from validity_cases import ENVS, expected_counters, fixture, multistart_case, top_id, wide_cvrp_case

pytestmark = pytest.mark.gpu


def device_instances(env, g):
    """The instance arrays of a group on the device, in the types the ops take."""
    d = {k: t(g[k]) for k in mk.INSTANCE_KEYS[env]}
    if env == "cvrptw":
        d["time_windows"] = d["time_windows"].to(torch.float32)
    return d


def counters(env, d, actions, inst):
    """The kernels' counters for `actions` (device [R, T]), row r judged by instance inst[r] (device index tensor), or by
    instance r % B where inst is None.  -> list of K ints."""
    from eam_rl4co_amd import ops

    actions = actions.contiguous()
    pick = (lambda x: x) if inst is None else (lambda x: x[inst].contiguous())
    if env == "tsp":
        return ops.check_solution("tsp", actions, num_loc=actions.shape[1]).tolist()
    if env in ("cvrp", "sdvrp"):
        return ops.check_solution(env, actions, pick(d["demand"]), pick(d["capacity"])).tolist()
    if env == "pctsp":
        return ops.check_solution("pctsp", actions, pick(d["real_prize"])).tolist()
    if env == "op":
        return ops.op_check_solution(actions, pick(d["locs"]), pick(d["max_length"])).tolist()
    late = ops.cvrptw_check_time(actions, pick(d["locs"]), pick(d["time_windows"]), pick(d["durations"])).tolist()
    assert late[1] == 0
    return ops.check_solution("cvrp", actions, pick(d["demand"]), pick(d["capacity"])).tolist() + late[:1]


def mixed_order(verdict):
    """Row indices with bad and valid rows alternating, so that the four waves of a block see different verdicts."""
    bad, ok = np.flatnonzero(verdict != 0).tolist(), np.flatnonzero(verdict == 0).tolist()
    out = []
    while bad or ok:
        for src in (bad, ok):
            if src:
                out.append(src.pop(0))
    return np.array(out)


@pytest.mark.parametrize("env", ENVS)
def test_counts_equal_the_recorded_verdicts(env):
    for i, g in enumerate(fixture(env)):
        d, a, inst = device_instances(env, g), t(g["actions"]), t(g["inst"])
        want = expected_counters(env, g)
        got = counters(env, d, a, inst)
        print(env, "group", i, "rows", tuple(g["actions"].shape), "counters", got, "recorded", want.sum(0).tolist())
        assert got == want.sum(0).tolist(), f"{env} group {i}"
        order = mixed_order(g["verdict"])
        R = order.size
        for n in (1, 3, 4, 5, 9, 4 * ((R - 1) // 4) + 1):
            for start in (0, 1, 2):
                rows = order[start:start + n]
                got = counters(env, d, a[t(rows)], inst[t(rows)])
                assert got == want[rows].sum(0).tolist(), f"{env} group {i}: rows {rows.tolist()}"


@pytest.mark.parametrize("env", ENVS)
def test_every_row_alone_gets_its_recorded_verdict(env):
    wrong = []
    for i, g in enumerate(fixture(env)):
        d, a, inst = device_instances(env, g), t(g["actions"]), t(g["inst"])
        want = expected_counters(env, g)
        for r in range(a.shape[0]):
            got = counters(env, d, a[r:r + 1], inst[r:r + 1])
            if got != want[r].tolist():
                wrong.append((i, r, str(g["cls"][r]), got, want[r].tolist()))
    print(env, "rows that differ (group, row, class, kernel, recorded):", wrong[:20])
    assert not wrong, f"{env}: {len(wrong)} rows differ, first {wrong[:5]}"


@pytest.mark.parametrize("env", ENVS[1:])            # TSP has no instance data: nothing depends on the mapping
@pytest.mark.parametrize("S", [3, 5])
def test_multistart_rows_read_instance_r_mod_B(env, S):
    sub, actions, right, wrong = multistart_case(env, S)
    got = counters(env, device_instances(env, sub), t(actions), None)
    print(env, "S", S, "kernel", got, "r % B", right.counters.sum(0).tolist(), "r // S", wrong.counters.sum(0).tolist())
    assert got == right.counters.sum(0).tolist()


@pytest.mark.parametrize("env", ["tsp", "cvrp"])
def test_rollout_finish_adds_the_same_counts(env):
    """The TSP / CVRP check behind eamrl_rollout_finish (the row function of eamrl_check_solution's kernel, called from the
    epilogue kernel): `bad +=`, with and without the log-likelihood and the reward."""
    from eam_rl4co_amd import ops

    rng = np.random.default_rng(5)
    seen_step64 = 0
    for i, g in enumerate(fixture(env)):
        a = t(g["actions"])
        R, T = a.shape
        M = T if env == "tsp" else g["demand"].shape[1] + 1
        locs = t(rng.random((R, M, 2), dtype=np.float32))
        logp = t(-rng.random((R, T), dtype=np.float32))
        demand = t(g["demand"][g["inst"]]) if env == "cvrp" else None
        vcap = t(g["capacity"][g["inst"]]) if env == "cvrp" else None
        want = expected_counters(env, g)
        seen_step64 += int((g["cls"] == "over_step64").sum())
        order = mixed_order(g["verdict"])
        for rows in (np.arange(R), order[:5], np.flatnonzero(g["cls"] == "over_step64")):
            if rows.size == 0:
                continue
            idx = t(rows)
            sel = lambda x: None if x is None else x[idx].contiguous()
            for lp, want_reward in ((logp, True), (None, True), (logp, False), (None, False)):
                bad = torch.tensor([7, 11], dtype=torch.int32, device=DEV)
                reward, ll = ops.rollout_finish(env, sel(locs), sel(a), sel(lp), sel(demand), sel(vcap),
                                                want_reward=want_reward, bad=bad)
                assert (reward is None) == (not want_reward) and (ll is None) == (lp is None)
                got = (bad.cpu().numpy() - (7, 11)).tolist()
                assert got == want[rows].sum(0).tolist(), f"{env} group {i} rows {rows[:8].tolist()} logp {lp is not None}"
        wrong = []
        for r in range(R):                   # and row by row
            bad = torch.zeros(2, dtype=torch.int32, device=DEV)
            ops.rollout_finish(env, locs[r:r + 1], a[r:r + 1], None, None if demand is None else demand[r:r + 1],
                               None if vcap is None else vcap[r:r + 1], want_reward=False, bad=bad)
            if bad.tolist() != want[r].tolist():
                wrong.append((i, r, str(g["cls"][r]), bad.tolist(), want[r].tolist()))
        assert not wrong, f"{env}: rows differ (group, row, class, kernel, recorded) {wrong[:5]}"
    assert env == "tsp" or seen_step64 > 0


@pytest.mark.parametrize("env", ENVS)
def test_out_of_range_ids_count_as_invalid_tours(env):
    """An id below 0 or above the top node is counted in the first counter and never used as an index (each kernel checks
    the id before it indexes with it); a launch on valid rows afterwards returns zeros."""
    from eam_rl4co_amd import ops

    groups = fixture(env)
    short = next(g for g in groups[1:] if g["actions"].shape[1] < 64)
    long = next(g for g in groups if g["actions"].shape[1] > 72)
    for gi, g in enumerate((short, long)):              # rows shorter and longer than 64 steps
        d, top = device_instances(env, g), top_id(env, g)
        T = g["actions"].shape[1]
        ok = np.flatnonzero(g["verdict"] == 0)[:4]
        assert ok.size == 4
        inst = t(g["inst"][ok])
        base = g["actions"][ok].copy()
        assert vr.VALID == 0 and (expected_counters(env, g)[ok] == 0).all()
        for pos in sorted({1, min(70, T - 2)}):
            a = base.copy()
            a[0, pos], a[1, pos], a[2, pos] = -1, top + 1, 2 ** 40           # row 3 stays valid
            got = counters(env, d, t(a), inst)
            want = [3, 0] if env != "cvrptw" else [3, 0, 3]
            assert got == want, f"{env} group {gi} position {pos}: {got}"
            if env in ("tsp", "cvrp"):
                R = a.shape[0]
                M = T if env == "tsp" else top + 1
                bad = torch.zeros(2, dtype=torch.int32, device=DEV)
                reward, _ = ops.rollout_finish(env, torch.rand(R, M, 2, device=DEV), t(a), None,
                                               d["demand"][inst].contiguous() if env == "cvrp" else None,
                                               d["capacity"][inst].contiguous() if env == "cvrp" else None, bad=bad)
                assert bad.tolist() == [3, 0] and bool(torch.isfinite(reward).all())
            assert counters(env, d, t(base), inst) == [0] * len(want)


def _td(env, g, rows, device_data):
    import eam_rl4co_amd as ea

    inst = t(g["inst"][rows])
    src = {("vehicle_capacity" if k == "capacity" else k): (v[inst].reshape(-1, 1) if k == "capacity" else v[inst].contiguous())
           for k, v in device_data.items()}
    if "locs" not in src:
        M = g["actions"].shape[1] if env == "tsp" else top_id(env, g) + 1
        src["locs"] = torch.rand(len(rows), M, 2, device=DEV)
    return ea.TensorDict(src, batch_size=[len(rows)])


@pytest.mark.parametrize("env", ENVS)
def test_env_api_raises_the_reference_messages(env):
    """env.check_solution_validity / env.get_reward: one row of every class among valid rows raises the recorded message
    (or nothing), and with two failing classes in one batch the message the reference would raise first wins."""
    import eam_rl4co_amd as ea

    groups = fixture(env)
    for cls in mk.CLASSES[env]:
        gi = next(i for i in (*range(1, len(groups)), 0) if (groups[i]["cls"] == cls).any())
        g = groups[gi]
        e = ea.get_env(env, generator_params=dict(num_loc=top_id(env, g) + (env == "tsp")))
        r = int(np.flatnonzero(g["cls"] == cls)[0])
        rows = np.concatenate([np.flatnonzero(g["verdict"] == 0)[:2], [r]])
        td, a = _td(env, g, rows, device_instances(env, g)), t(g["actions"][rows])
        v = int(g["verdict"][r])
        if v == 0:
            e.check_solution_validity(td, a)
            if env in ("tsp", "cvrp"):
                assert e.get_reward(td, a).shape == (3,)
            continue
        with pytest.raises(AssertionError, match=vr.MESSAGE[env][v]):
            e.check_solution_validity(td, a)
        with pytest.raises(AssertionError, match=vr.MESSAGE[env][v]):
            e.get_reward(td, a)
    # two classes in one batch: the lower verdict code is the assertion the reference reaches first
    for g in groups[1:6]:
        codes = [c for c in sorted(vr.MESSAGE[env]) if (g["verdict"] == c).any()]
        if len(codes) < 2:
            continue
        e = ea.get_env(env, generator_params=dict(num_loc=top_id(env, g) + (env == "tsp")))
        for lo in codes:
            for hi in codes:
                if lo >= hi:
                    continue
                rows = np.array([np.flatnonzero(g["verdict"] == hi)[0], np.flatnonzero(g["verdict"] == 0)[0],
                                 np.flatnonzero(g["verdict"] == lo)[0]])
                with pytest.raises(AssertionError, match=vr.MESSAGE[env][lo]):
                    e.check_solution_validity(_td(env, g, rows, device_instances(env, g)), t(g["actions"][rows]))


def test_cvrp_wide_graph_reaches_the_high_bitmap_words():
    from eam_rl4co_amd import ops

    demand, cap, actions = wide_cvrp_case()
    want = vr.cvrp(demand, cap, actions).counters
    assert want.tolist() == [[0, 0], [1, 0], [1, 0], [0, 1]]
    d, c, a = t(demand), t(cap), t(actions)
    assert ops.check_solution("cvrp", a, d, c).tolist() == [2, 1]
    locs = torch.rand(4, 1001, 2, device=DEV)
    bad = torch.zeros(2, dtype=torch.int32, device=DEV)
    ops.rollout_finish("cvrp", locs, a, None, d, c, want_reward=False, bad=bad)
    assert bad.tolist() == [2, 1]
    for r in range(4):
        assert ops.check_solution("cvrp", a[r:r + 1], d[r:r + 1], c[r:r + 1]).tolist() == want[r].tolist(), r
        bad.zero_()
        ops.rollout_finish("cvrp", locs[r:r + 1], a[r:r + 1], None, d[r:r + 1], c[r:r + 1], want_reward=False, bad=bad)
        assert bad.tolist() == want[r].tolist(), r
