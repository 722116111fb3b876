"""GPU: top-k / top-p rollouts on the register-resident kernel (k_rollout_resident<..., FILT = true>,
csrc/rollout_resident.hip) -- stage D6b of the step kernel inside the resident finish.

Everything is compared bit for bit: with a loop of fused decode steps (k_decode_step, where the filter is defined and
pinned to the reference by tests/test_gpu_filter.py), with the streaming kernel on the same inputs, and on the crafted rows
of tests/golden/filter_cases.npz with the reference's recorded verdicts.  Every rollout case first asks ops.rollout_kernel
-- the function the dispatcher branches on -- that the call under test really runs on the resident kernel, so no case can
pass by taking the old path.

Sizes are the smallest at which a code path of the filter stage can go wrong: 20 (one partial block of lanes), 64, 65
(the second node of a lane begins), 100, 112 (last supported; CVRP-111), and every (chunk stride, chunk registers) variant
of the filtering instantiations (8/8: <= 32 nodes, 16/16: <= 64, 28/26: <= 104, 28/28: <= 112).
"""
import functools

import numpy as np
import pytest
import torch

import filter_cases as fc
import make_golden_filter as mk
from test_gpu_filter import _instance, device_cache, step
from test_gpu_parity import DEV, assert_bits_equal, make_policy, t

pytestmark = pytest.mark.gpu

CASES = fc.load_cases()
FILTERS = [(0, 0.8), (5, 0.0), (6, 0.9)]
ST_STEP_OVERRUN = 4


class forced:
    """eamrl_debug_set(key, 1) for the duration of a block (1: streaming kernel, 6: no start loop in the resident kernel)."""

    def __init__(self, key):
        self.key = key

    def __enter__(self):
        from eam_rl4co_amd import _lib

        assert _lib.load().eamrl_debug_set(self.key, 1) == 0

    def __exit__(self, *exc):
        from eam_rl4co_amd import _lib

        _lib.load().eamrl_debug_set(self.key, 0)


@functools.lru_cache(maxsize=None)
def policy(env_name):
    return make_policy("am_" + env_name)


@functools.lru_cache(maxsize=None)
def problem(env_name, N, B):
    """(td on the device, decoder cache) of B seeded instances; computed once and shared, never modified."""
    pol = policy(env_name)
    _, td_cpu, _, _ = _instance(env_name, N, B, 200 + N)
    td = td_cpu.to(DEV)
    with torch.no_grad():
        emb, _ = pol.encoder(td)
        cache = pol.decoder._precompute_cache(emb)
    return td, cache


def fresh_state(env_name, td, S):
    from eam_rl4co_amd.policy import _env_step_, state_from_td

    st = state_from_td(env_name, td, S)
    if S:       # select_start_nodes: row s * B + b starts at node s (TSP) / s + 1 (depot envs)
        B = td["locs"].shape[0]
        start = torch.arange(S, device=DEV).repeat_interleave(B) + (0 if env_name == "tsp" else 1)
        _env_step_(st, start)
    return st


def assert_resident(env_name, cache, R, t_max, top_k, top_p):
    from eam_rl4co_amd import ops

    got = ops.rollout_kernel(env_name, cache, R, t_max, top_k=top_k, top_p=top_p)
    assert got == "resident", f"{env_name} M {cache.M} R {R} top_k {top_k} top_p {top_p} runs on {got}"


class kernels_of_rollouts:
    """Records, for every ops.rollout call made inside the block (the policy's own calls included), the kernel that call
    resolves to: ops.rollout_kernel asked with the call's own state, cache, t_max and filter."""

    def __init__(self, monkeypatch):
        self.monkeypatch, self.seen = monkeypatch, []

    def __enter__(self):
        from eam_rl4co_amd import ops

        real = ops.rollout

        def spy(st, cache, mode="greedy", noise=None, given=None, clip=10.0, temp=1.0, t_max=None, top_k=0, top_p=0.0, **kw):
            tm = t_max if noise is None else noise.shape[1]
            self.seen.append((ops.rollout_kernel(st, cache, st.R, tm, top_k=top_k, top_p=top_p), st.R, top_k, top_p))
            return real(st, cache, mode, noise=noise, given=given, clip=clip, temp=temp, t_max=t_max, top_k=top_k, top_p=top_p, **kw)

        self.monkeypatch.setattr(ops, "rollout", spy)
        return self.seen

    def __exit__(self, *exc):
        self.monkeypatch.undo()


def against_the_step_loop(env_name, N, S, top_k, top_p, temp=1.0, clip=10.0, neutral=False, more_modes=False):
    from eam_rl4co_amd import ops
    from eam_rl4co_amd.policy import _max_decode_steps

    B = 2
    pol = policy(env_name)
    td, cache = problem(env_name, N, B)
    M = td["action_mask"].shape[1]
    R = B * max(S, 1)
    t_max = _max_decode_steps(env_name, M, 1 if S else 0)
    assert_resident(env_name, cache, R, t_max, top_k, top_p)
    fresh = lambda: fresh_state(env_name, td, S)
    noise = ops.exp1_noise(20261018 + N, R, t_max, M, DEV)
    kw = dict(clip=clip, temp=temp, top_k=top_k, top_p=top_p)

    acts, lps, _, T, status = pol._rollout_stepwise(fresh(), cache, "sampling", noise, None, clip, temp, t_max, top_k, top_p)
    assert status == 0 and T > 0
    a, lp, info = ops.rollout(fresh(), cache, "sampling", noise=noise, t_max=t_max, **kw)
    assert info.cpu().tolist() == [T, 0]
    assert_bits_equal(a[:, :T], acts, "sampling: actions")
    assert_bits_equal(lp[:, :T], lps, "sampling: log-probs")
    assert torch.isfinite(lp).all()
    a0, lp0, info0 = ops.rollout(fresh(), cache, "sampling", noise=noise, clip=clip, temp=temp, t_max=t_max)
    if neutral:     # top_k >= M is clamped to M and keeps every entry: the filtering variant gives the unfiltered rollout
        assert_bits_equal(a, a0, "top_k >= M: actions")
        assert_bits_equal(lp, lp0, "top_k >= M: log-probs")
    else:
        assert not torch.equal(lp0[:, :T], lps), "the filter changed nothing: the case does not test it"
    if top_k == 1:  # only the largest logit survives: the greedy tour, every log-prob exactly 0
        g, _, _ = ops.rollout(fresh(), cache, "greedy", clip=clip, temp=temp, t_max=t_max)
        assert torch.equal(a, g) and bool((lp == 0).all())
    if not more_modes:
        return
    # greedy under a filter
    ga, glp, _, gT, gstatus = pol._rollout_stepwise(fresh(), cache, "greedy", None, None, clip, temp, t_max, top_k, top_p)
    a, lp, info = ops.rollout(fresh(), cache, "greedy", t_max=t_max, **kw)
    assert info.cpu().tolist() == [gT, gstatus] and gstatus == 0
    assert_bits_equal(a[:, :gT], ga, "greedy: actions")
    assert_bits_equal(lp[:, :gT], glp, "greedy: log-probs")
    # evaluate: the filtered sample's own actions (all kept: finite log-probs, equal to the sampling run's) ...
    given = acts.contiguous()
    ea, elp, _, eT, estatus = pol._rollout_stepwise(fresh(), cache, "evaluate", None, given, clip, temp, T, top_k, top_p)
    a, lp, info = ops.rollout(fresh(), cache, "evaluate", given=given, t_max=T, **kw)
    assert info.cpu().tolist() == [eT, estatus] and (eT, estatus) == (T, 0)
    assert_bits_equal(a[:, :T], ea, "evaluate: actions")
    assert_bits_equal(lp[:, :T], elp, "evaluate: log-probs")
    assert_bits_equal(lp[:, :T], lps, "evaluate == the sampling run's log-probs")
    # ... and the unfiltered sample's: a given action the filter removed is a feasible action with log-prob -inf
    T0 = int(info0[0])
    given = a0[:, :T0].contiguous()
    ea, elp, _, eT, estatus = pol._rollout_stepwise(fresh(), cache, "evaluate", None, given, clip, temp, T0, top_k, top_p)
    a, lp, info = ops.rollout(fresh(), cache, "evaluate", given=given, t_max=T0, **kw)
    assert info.cpu().tolist() == [eT, estatus]
    assert_bits_equal(a[:, :eT], ea, "evaluate (unfiltered actions): actions")
    assert_bits_equal(lp[:, :eT], elp, "evaluate (unfiltered actions): log-probs")
    assert bool(torch.isneginf(elp).any()), "no given action was filtered out: the case does not test it"


# ---------------------------------------------------------------------------------------------------------
# 1. resident FILT == loop of fused steps
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k,top_p", FILTERS)
@pytest.mark.parametrize("env_name,N", [("tsp", 20), ("tsp", 64), ("tsp", 65), ("tsp", 100), ("tsp", 112),
                                        ("cvrp", 20), ("cvrp", 100), ("cvrp", 111)])
def test_filtered_resident_rollout_equals_the_step_loop(env_name, N, top_k, top_p):
    against_the_step_loop(env_name, N, 0, top_k, top_p)


@pytest.mark.parametrize("env_name", ["sdvrp", "pctsp", "op", "cvrptw"])
def test_filtered_resident_rollout_equals_the_step_loop_sibling_envs(env_name):
    against_the_step_loop(env_name, 20, 0, 6, 0.9)


@pytest.mark.parametrize("env_name,N", [("tsp", 65), ("cvrp", 100)])
@pytest.mark.parametrize("what", ["top_k >= M", "top_k = 1", "temperature 0.5", "no tanh clipping"])
def test_filtered_resident_rollout_settings(env_name, N, what):
    M = N + (env_name != "tsp")
    if what == "top_k >= M":
        against_the_step_loop(env_name, N, 0, M, 0.0, neutral=True)
        against_the_step_loop(env_name, N, 0, M + 7, 0.0, neutral=True)
    elif what == "top_k = 1":
        against_the_step_loop(env_name, N, 0, 1, 0.0)
    elif what == "temperature 0.5":
        against_the_step_loop(env_name, N, 0, 0, 0.8, temp=0.5)
    else:
        against_the_step_loop(env_name, N, 0, 5, 0.0, clip=0.0)


@pytest.mark.parametrize("top_k,top_p", FILTERS)
@pytest.mark.parametrize("env_name,N", [("tsp", 65), ("cvrp", 100)])
def test_filtered_resident_multistart_equals_the_step_loop(env_name, N, top_k, top_p):
    against_the_step_loop(env_name, N, 3, top_k, top_p)


@pytest.mark.parametrize("top_k,top_p", [(5, 0.0), (6, 0.9)])
@pytest.mark.parametrize("env_name,N", [("tsp", 65), ("cvrp", 100)])
def test_filtered_resident_greedy_and_evaluate_equal_the_step_loop(env_name, N, top_k, top_p):
    against_the_step_loop(env_name, N, 0, top_k, top_p, more_modes=True)


# ---------------------------------------------------------------------------------------------------------
# 2. resident FILT == streaming kernel
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_name,N,B,S", [("tsp", 100, 8, 0), ("cvrp", 100, 8, 0), ("tsp", 100, 4, 5), ("cvrp", 100, 4, 5),
                                            ("tsp", 20, 128, 20), ("cvrp", 20, 128, 20)])
def test_filtered_resident_rollout_equals_the_streaming_kernel(env_name, N, B, S):
    """The last two cases make a workgroup roll out several starts one after the other on its register-resident operands
    (the start loop re-initialises the row state in LDS between them): the launcher gives an instance G = min(S,
    ceil(2048 / B)) workgroups, so B = 128 with S = 20 starts leaves G = 16 < S and four workgroups of every instance
    take a second start.  In the other multistart cases G = S."""
    from eam_rl4co_amd import ops
    from eam_rl4co_amd.policy import _max_decode_steps

    td, cache = problem(env_name, N, B)
    M = td["action_mask"].shape[1]
    R = B * max(S, 1)
    assert (S > -(-2048 // B)) == (B == 128)
    t_max = _max_decode_steps(env_name, M, 1 if S else 0)
    noise = ops.exp1_noise(77, R, t_max, M, DEV)
    for top_k, top_p in FILTERS:
        assert_resident(env_name, cache, R, t_max, top_k, top_p)
        run = lambda: ops.rollout(fresh_state(env_name, td, S), cache, "sampling", noise=noise, t_max=t_max, top_k=top_k,
                                  top_p=top_p)
        a, lp, info = run()
        with forced(1):
            assert ops.rollout_kernel(env_name, cache, R, t_max, top_k=top_k, top_p=top_p) == "stream"
            sa, slp, sinfo = run()
        assert info.cpu().tolist() == sinfo.cpu().tolist() and int(info[1]) == 0
        assert_bits_equal(a, sa, f"actions, top_k {top_k} top_p {top_p}")
        assert_bits_equal(lp, slp, f"log-probs, top_k {top_k} top_p {top_p}")


# ---------------------------------------------------------------------------------------------------------
# 3. ties and the boundary: the crafted rows of the golden through one-step rollouts
# ---------------------------------------------------------------------------------------------------------
def test_crafted_rows_through_one_step_resident_rollouts():
    """A crafted row (tests/filter_cases.py) as a TSP instance of M nodes rolled out for one step in evaluate mode, one
    rollout row per node with that node as the given action (R = M rows of one instance): a row's log-prob is finite iff
    its node was kept, so one launch returns the whole verdict.  Compared with the recorded verdicts, with the float64
    log-softmax over the kept set within 1e-5 (the tolerance of test_gpu_filter.py) and bit for bit with the step kernel.
    Both forms of the resident kernel run: the start loop (R = M rows are a multistart batch) and one workgroup per row.
    topp0 / topp1 carry neutral settings, which are unfiltered calls (test 4), and the rows of 128 and 256 nodes are
    beyond the filtering variant; every other crafted row takes part."""
    from eam_rl4co_amd import ops

    names = []
    for i, c in enumerate(CASES):
        M = c["x"].size
        if not c["crafted"] or M > 112 or not (c["top_k"] > 0 or 0.0 < c["top_p"] < 1.0):
            continue
        names.append(c["name"])
        cache, mask = fc.crafted_cache(c, i)
        dc = device_cache(cache)
        feas = mask[0] != 0
        st1 = ops.RolloutState("tsp", 1, M, DEV)
        st1.mask = t(mask != 0)
        _, _, step_lps, lgs = step(st1, dc, "greedy", None, c["top_k"], c["top_p"])
        assert np.array_equal(lgs[0], c["x"]), (c["name"], "the synthetic cache does not give the recorded row")
        given = np.where(feas, np.arange(M), int(np.flatnonzero(feas)[0]))[:, None]      # masked nodes: ask for a feasible one
        assert_resident("tsp", dc, M, 1, c["top_k"], c["top_p"])
        for single in (False, True):
            st = ops.RolloutState("tsp", M, M, DEV)
            st.mask = t(np.repeat(mask != 0, M, 0))
            run = lambda: ops.rollout(st, dc, "evaluate", given=t(given), clip=0.0, temp=1.0, t_max=1, top_k=c["top_k"],
                                      top_p=c["top_p"])
            if single:
                with forced(6):
                    a, lp, info = run()
            else:
                a, lp, info = run()
            assert int(info[0]) == 1 and int(info[1]) & ~ST_STEP_OVERRUN == 0, (c["name"], info.cpu().tolist())
            assert np.array_equal(a.cpu().numpy(), given)
            lp = lp.cpu().numpy()[:, 0]
            keep = np.isfinite(lp) & feas
            fc.check_keep(c, keep, "resident kernel")
            row = np.where(feas, lp, -np.inf).astype(np.float32)
            fc.check_logp(row, keep, c["x"], 1e-5, c["name"])
            assert_bits_equal(row, step_lps[0], f"{c['name']}: log-probs vs the step kernel")
    want = [n for n, a, k, p in mk.crafted() if len(a) <= 112 and (k > 0 or 0.0 < p < 1.0)]
    assert names == want
    # equal logits at the top-k edge / inside the nucleus (ranked by index) / a running sum exactly on float32(1 - top_p)
    for n in ("topk2_tie2", "topk2_tie3_across64", "straddle_low_group", "straddle_across64", "uniform5_p0.8", "uniform4_p0.75"):
        assert n in names


# ---------------------------------------------------------------------------------------------------------
# 4. neutral settings
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 3])
def test_neutral_settings_run_the_unfiltered_kernel_and_change_nothing(S):
    from eam_rl4co_amd import ops
    from eam_rl4co_amd.policy import _max_decode_steps

    B = 2
    td, cache = problem("tsp", 65, B)
    M, R = 65, B * max(S, 1)
    t_max = _max_decode_steps("tsp", M, 1 if S else 0)
    noise = ops.exp1_noise(5, R, t_max, M, DEV)
    plain = ops.rollout_kernel("tsp", cache, R, t_max)
    assert plain == ("ms_mfma" if S else "resident")
    base = ops.rollout(fresh_state("tsp", td, S), cache, "sampling", noise=noise, t_max=t_max)
    for top_k, top_p in ((0, 0.0), (0, 1.0)):
        assert ops.rollout_kernel("tsp", cache, R, t_max, top_k=top_k, top_p=top_p) == plain
        got = ops.rollout(fresh_state("tsp", td, S), cache, "sampling", noise=noise, t_max=t_max, top_k=top_k, top_p=top_p)
        for x, y, what in zip(got, base, ("actions", "log-probs", "info")):
            assert_bits_equal(x, y, f"top_k {top_k} top_p {top_p}: {what}")


# ---------------------------------------------------------------------------------------------------------
# 5. policy level
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
def test_policy_top_p_sampling_equals_the_streaming_run(env_name, monkeypatch):
    from eam_rl4co_amd import ops
    from eam_rl4co_amd.policy import _max_decode_steps

    B, N = 16, 50
    pol = policy(env_name)
    env, td_cpu, _, _ = _instance(env_name, N, B, 31)
    td = td_cpu.to(DEV)
    M = td["action_mask"].shape[1]
    t_max = _max_decode_steps(env_name, M, 0)
    with torch.no_grad():
        emb, _ = pol.encoder(td)
        assert_resident(env_name, pol.decoder._precompute_cache(emb), B, t_max, 0, 0.9)
    noise = torch.empty(B, t_max, M).exponential_(1, generator=torch.Generator().manual_seed(9)).to(DEV)

    def run():
        with torch.no_grad():
            return pol(td.clone(), env, phase="test", decode_type="sampling", top_p=0.9, noise=noise)

    with kernels_of_rollouts(monkeypatch) as seen:
        out = run()
    assert seen == [("resident", B, 0, 0.9)], seen          # the policy's own call, not a rebuilt one
    with forced(1), kernels_of_rollouts(monkeypatch) as seen:
        ref = run()
    assert seen == [("stream", B, 0, 0.9)], seen
    plain = None
    with torch.no_grad():
        plain = pol(td.clone(), env, phase="test", decode_type="sampling", noise=noise)
    for k in ("actions", "reward", "log_likelihood"):
        assert_bits_equal(out[k], ref[k], k)
    assert out["actions"].shape[0] == B
    assert torch.isfinite(out["log_likelihood"]).all()
    assert out["actions"].shape != plain["actions"].shape or not torch.equal(out["actions"], plain["actions"])


def test_sampling_eval_top_p_equals_the_streaming_run(monkeypatch):
    from eam_rl4co_amd.eval import SamplingEval

    pol = policy("tsp")
    env, td_cpu, _, _ = _instance("tsp", 20, 4, 41)
    td = td_cpu.to(DEV)
    ev = SamplingEval(env, samples=8, top_p=0.9)

    def run():
        torch.manual_seed(123)          # the random start nodes and the rollout's seed come from torch's generators
        with torch.no_grad():
            return ev._inner(pol, td)

    with kernels_of_rollouts(monkeypatch) as seen:
        a, r = run()
    assert seen == [("resident", 4 * 8, 0, 0.9)], seen      # 8 samples of 4 instances: the resident kernel's start loop
    with forced(1), kernels_of_rollouts(monkeypatch) as seen:
        sa, sr = run()
    assert seen == [("stream", 4 * 8, 0, 0.9)], seen
    assert_bits_equal(r, sr, "best rewards")
    assert_bits_equal(a, sa, "best actions")
    assert r.shape[0] == 4 and torch.isfinite(r).all()


# ---------------------------------------------------------------------------------------------------------
# 6. non-default stream and graph capture
# ---------------------------------------------------------------------------------------------------------
def test_filtered_resident_rollout_on_a_side_stream_and_in_a_captured_graph():
    from eam_rl4co_amd import ops

    B = 8
    td, cache = problem("tsp", 100, B)
    M = t_max = 100
    assert_resident("tsp", cache, B, t_max, 0, 0.9)
    noise = ops.exp1_noise(11, B, t_max, M, DEV)
    run = lambda: ops.rollout(fresh_state("tsp", td, 0), cache, "sampling", noise=noise, t_max=t_max, top_p=0.9)
    a, lp, info = run()
    assert info.cpu().tolist() == [t_max, 0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sa, slp, sinfo = run()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(sa, a) and torch.equal(slp, lp) and torch.equal(sinfo, info)

    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ga, glp, ginfo = run()
    for _ in range(2):
        ga.zero_(), glp.zero_(), ginfo.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ga, a) and torch.equal(glp, lp) and torch.equal(ginfo, info)
