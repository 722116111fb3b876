"""TSP 2-opt local search on the GPU (eamrl_tsp_two_opt, TSPEnv.local_search): identical tours and sweep counts to the
reference on the recorded fixtures (tests/golden/ls_*.npz), and to the test-side restatement (tests/two_opt_ref.py, pinned
to the same fixtures by test_host_local_search.py) at full size and around every size at which the launch switches variant.
All comparisons are exact."""
import numpy as np
import pytest
import torch

import two_opt_ref as ref
from _util import golden
from test_gpu_parity import DEV, make_policy, t
from test_host_local_search import EXPECTED

pytestmark = pytest.mark.gpu


def _td(locs, distances=None):
    import eam_rl4co_amd as ea

    src = {"locs": t(locs)}
    if distances is not None:
        src["distances"] = t(distances)
    return ea.TensorDict(src, batch_size=[locs.shape[0]])


def _run_both(locs, actions, max_it, distances=None):
    """TSPEnv.local_search and ops.tsp_two_opt on the same inputs -> (tours, iters) as numpy, after the contract checks."""
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import ops

    a = t(actions)
    keep = a.clone()
    td = _td(locs, distances)
    out = ea.TSPEnv.local_search(td, a, max_iterations=max_it)
    if distances is None:
        tours, iters, status = ops.tsp_two_opt(a, locs=td["locs"], max_iterations=max_it)
    else:
        tours, iters, status = ops.tsp_two_opt(a, distances=td["distances"], max_iterations=max_it)
    for o in (out, tours):
        assert o.dtype == torch.int64 and o.shape == a.shape and o.device == a.device
        assert o.data_ptr() != a.data_ptr()
    assert iters.dtype == torch.int32 and iters.shape == (a.shape[0],) and status.dtype == torch.int32
    assert int(status.item()) == 0
    assert torch.equal(a, keep), "the input tours were modified"
    assert torch.equal(out, tours)
    return tours.cpu().numpy(), iters.cpu().numpy()


def _check_improved(locs, actions, tours):
    import eam_rl4co_amd as ea

    n = actions.shape[1]
    assert np.array_equal(np.sort(tours, axis=1), np.broadcast_to(np.arange(n), tours.shape)), "not permutations"
    assert np.array_equal(tours[:, 0], actions[:, 0]), "position 0 moved"
    env = ea.get_env("tsp", generator_params=dict(num_loc=n))
    td = _td(locs)
    before = env.get_reward(td, t(actions), check_solution=False)
    after = env.get_reward(td, t(tours), check_solution=False)
    assert bool((after >= before).all()), "a tour got longer"


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_fixtures_equal_the_reference(name):
    fx = golden(name)
    tours, iters = _run_both(fx["locs"], fx["actions"], int(fx["max_iterations"]), fx.get("distances"))
    print(name, "sweeps", iters.tolist(), "reference", fx["iters"].tolist())
    assert np.array_equal(tours, fx["tours"])
    assert np.array_equal(iters, fx["iters"])


def _against_restatement(locs, actions, max_it, distances=None, what=""):
    tours, iters = _run_both(locs, actions, max_it, distances)
    want_t, want_i = ref.two_opt_batch(actions, locs=locs, distances=distances, max_iterations=max_it)
    rows = np.flatnonzero((tours != want_t).any(axis=1) | (iters != want_i))
    print(f"{what}: rows {actions.shape[0]} n {actions.shape[1]} sweeps {int(iters.sum())} (restatement {int(want_i.sum())}) "
          f"differing rows {rows.size}")
    assert rows.size == 0, f"{what}: rows {rows[:8].tolist()} differ from the restatement"
    if distances is None:
        _check_improved(locs, actions, tours)
    return tours, iters


def _greedy_tours(locs):
    import eam_rl4co_amd as ea

    n = locs.shape[1]
    env = ea.get_env("tsp", generator_params=dict(num_loc=n))
    td = env.reset(ea.TensorDict({"locs": torch.from_numpy(locs)}, batch_size=[locs.shape[0]])).to(DEV)
    pol = make_policy("am_tsp")
    with torch.no_grad():
        out = pol(td, env, phase="test", decode_type="greedy")
    return out["actions"].cpu().numpy()


def test_full_size_tsp100_policy_tours():
    locs, _, max_it = ref.full_size_case("tsp100")
    _against_restatement(locs, _greedy_tours(locs), max_it, what="1024 x TSP-100, greedy tours")


def test_full_size_tsp100_random_permutations():
    locs, perms, max_it = ref.full_size_case("tsp100")
    _, iters = _against_restatement(locs, perms, max_it, what="1024 x TSP-100, random permutations")
    assert iters.min() > 50                    # a random TSP-100 tour takes about n sweeps


@pytest.mark.parametrize("name", ["tsp20", "tsp200", "tsp1024_cap20"])
def test_full_size_other_shapes(name):
    locs, perms, max_it = ref.full_size_case(name)
    _, iters = _against_restatement(locs, perms, max_it, what=name)
    if name == "tsp1024_cap20":
        assert (iters == 20).all()


def test_each_side_of_every_variant_threshold():
    """The launch picks its workgroup size by n (64 threads up to TWO_OPT_WAVE_MAX, 256 up to TWO_OPT_BLOCK256_MAX, 1024 above)
    and keeps a `distances` matrix in LDS up to TWO_OPT_LDS_MATRIX_MAX nodes, in global memory above."""
    from eam_rl4co_amd import ops

    assert (ops.TWO_OPT_WAVE_MAX, ops.TWO_OPT_BLOCK256_MAX, ops.TWO_OPT_LDS_MATRIX_MAX) == (48, 256, 120)
    rng = np.random.default_rng(11)
    for n in (ops.TWO_OPT_WAVE_MAX, ops.TWO_OPT_WAVE_MAX + 1, ops.TWO_OPT_BLOCK256_MAX, ops.TWO_OPT_BLOCK256_MAX + 1):
        B, cap = (6, 1000) if n < 100 else (3, 40)
        locs = rng.random((B, n, 2), dtype=np.float32)
        perms = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int64)
        _against_restatement(locs, perms, cap, what=f"coordinates, n = {n}")
    # asymmetric matrices: both workgroup sizes of the LDS variant, both sides of the LDS / global switch, and the 1024-thread
    # global variant
    for n in (ops.TWO_OPT_WAVE_MAX, ops.TWO_OPT_WAVE_MAX + 1, ops.TWO_OPT_LDS_MATRIX_MAX, ops.TWO_OPT_LDS_MATRIX_MAX + 1,
              ops.TWO_OPT_BLOCK256_MAX, ops.TWO_OPT_BLOCK256_MAX + 1):
        B, cap = 3, 40
        locs = rng.random((B, n, 2), dtype=np.float32)
        dist = rng.random((B, n, n), dtype=np.float32)
        perms = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int64)
        _against_restatement(locs, perms, cap, distances=dist, what=f"asymmetric distances, n = {n}")
    # a symmetric matrix made of the restatement's own distances gives the tours of the coordinate path
    locs = rng.random((4, 60, 2), dtype=np.float32)
    perms = np.stack([rng.permutation(60) for _ in range(4)]).astype(np.int64)
    a, ia = _run_both(locs, perms, 1000)
    b, ib = _run_both(locs, perms, 1000, distances=ref.distance_matrix(locs))
    assert np.array_equal(a, b) and np.array_equal(ia, ib)


def test_two_nodes_and_zero_iterations():
    from eam_rl4co_amd import ops

    locs = np.random.default_rng(3).random((5, 2, 2), dtype=np.float32)
    acts = np.array([[0, 1], [1, 0], [0, 1], [1, 0], [1, 0]], dtype=np.int64)
    tours, iters = _run_both(locs, acts, 1000)
    assert np.array_equal(tours, acts) and (iters == 1).all()
    locs, perms, _ = ref.full_size_case("tsp20")
    a = t(perms)
    tours, iters, status = ops.tsp_two_opt(a, locs=t(locs), max_iterations=0)
    assert torch.equal(tours, a) and tours.data_ptr() != a.data_ptr()
    assert int(iters.abs().sum()) == 0 and int(status.item()) == 0
    # the env method takes what the reference's takes: any integer dtype of the tours, any float dtype of the coordinates
    import eam_rl4co_amd as ea

    td32 = _td(locs)
    want = ea.TSPEnv.local_search(td32, a)
    got = ea.TSPEnv.local_search(ea.TensorDict({"locs": td32["locs"].double()}, batch_size=[locs.shape[0]]), a.int())
    assert got.dtype == torch.int64 and torch.equal(got, want)


def test_rows_that_are_not_permutations():
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import ops

    locs, perms, max_it = ref.full_size_case("tsp20")
    locs, perms = locs[:16], perms[:16].copy()
    perms[5, 7] = perms[5, 3]                                # one duplicated node in one row
    a = t(perms)
    with pytest.raises(ValueError, match="not permutations"):
        ea.TSPEnv.local_search(_td(locs), a)
    tours, iters, status = ops.tsp_two_opt(a, locs=t(locs), max_iterations=max_it)
    assert int(status.item()) == 1
    tours, iters = tours.cpu().numpy(), iters.cpu().numpy()
    assert np.array_equal(tours[5], perms[5]) and iters[5] == 0
    others = np.arange(16) != 5
    want_t, want_i = ref.two_opt_batch(perms[others], locs=locs[others], max_iterations=max_it)
    assert np.array_equal(tours[others], want_t) and np.array_equal(iters[others], want_i)
    assert (tours[others] != perms[others]).any(axis=1).all()
    # ids outside 0..n-1 never index anything: the rows pass through and are counted
    perms[2, 0], perms[9, 4] = 20, -1
    tours, iters, status = ops.tsp_two_opt(t(perms), locs=t(locs), max_iterations=max_it)
    assert int(status.item()) == 3
    assert np.array_equal(tours.cpu().numpy()[[2, 5, 9]], perms[[2, 5, 9]])
    with pytest.raises(ValueError):
        ops.tsp_two_opt(a, max_iterations=3)                 # neither locs nor distances
    with pytest.raises(ValueError):
        ops.tsp_two_opt(a, locs=t(locs), distances=t(ref.distance_matrix(locs)))


def test_non_default_stream_and_graph_capture_after_a_greedy_rollout():
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import ops

    locs = ref.full_size_case("tsp100")[0][:64]
    n = locs.shape[1]
    env = ea.get_env("tsp", generator_params=dict(num_loc=n))
    td = env.reset(ea.TensorDict({"locs": torch.from_numpy(locs)}, batch_size=[64])).to(DEV)
    pol = make_policy("am_tsp")
    with torch.no_grad():
        greedy = pol(td.clone(), env, phase="test", decode_type="greedy")["actions"]
    eager, eager_iters, _ = ops.tsp_two_opt(greedy, locs=td["locs"])
    want_t, want_i = ref.two_opt_batch(greedy.cpu().numpy(), locs=locs)
    assert np.array_equal(eager.cpu().numpy(), want_t) and np.array_equal(eager_iters.cpu().numpy(), want_i)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s_tours, s_iters, s_status = ops.tsp_two_opt(greedy, locs=td["locs"])
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(s_tours, eager) and torch.equal(s_iters, eager_iters) and int(s_status.item()) == 0

    # rollout + polish in one captured graph: the device half of the policy's forward, then the 2-opt launch on its tours
    kw = dict(phase="test", calc_reward=True, return_actions=True, return_entropy=False, return_hidden=False,
              return_init_embeds=False, return_sum_log_likelihood=True, actions=None, max_steps=1_000_000, decode_type="greedy")
    static_td = td.clone()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            pol._finish(pol._enqueue(static_td, env, **kw))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        pending = pol._enqueue(static_td, env, **kw)
        rolled = pending["actions_pad"][:, :n].contiguous()
        g_tours, g_iters, g_status = ops.tsp_two_opt(rolled, locs=static_td["locs"])
    for _ in range(2):
        g_status.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(rolled, greedy)
        assert torch.equal(g_tours, eager) and torch.equal(g_iters, eager_iters) and int(g_status.item()) == 0
