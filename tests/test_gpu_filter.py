"""GPU: the top-k / top-p filtering of a decode step (stage D6b of csrc/decode_step.hip, shared by the step kernel and the
streaming rollout kernel) against the verdicts recorded from the reference's own process_logits
(tests/golden/filter_cases.npz), against the plain restatement tests/filter_ref.py applied to the kernel's own logits, and
bit for bit against the CPU oracle, at the sizes where the filter leaves its first 64-entry block (65), its second wave-sum
partial (129) and the first pass of its block-stride loops (257).

Tolerances: keep sets are compared exactly (random rows under the margin rule of make_golden_filter.py); kept log-probs are
within 1e-5 of the float64 log-softmax over the kept set, the tolerance test_policy_forward_reproduces_reference_tours uses
against the reference; everything compared with the oracle or between two kernels is compared bit for bit.
"""
import math

import numpy as np
import pytest
import torch

import filter_cases as fc
import filter_ref as fr
import make_golden_filter as mk
from _util import golden_weights, instance_from_td
from test_gpu_parity import DEV, assert_bits_equal, make_policy, t

pytestmark = pytest.mark.gpu

CASES = fc.load_cases()


def device_cache(cache, planes=False):
    """ops.DecodeCache of a synthetic TSP cache (dict of numpy arrays, tests/filter_cases.py), slot- or plane-major."""
    from eam_rl4co_amd import ops

    parts = [cache[n] if n != "L" else np.zeros_like(cache["K"]) for n in ("K", "V", "L", "Pa", "Pb", "Lp")]
    buf = np.stack(parts, 0) if planes else np.concatenate(parts, -1)
    return ops.DecodeCache("tsp", t(buf), t(cache["cvec"]), t(cache["gctx"]), None, fc.H, embed_dim=fc.E)


def tsp_states(oracle, mask):
    """(oracle state, device state) of a TSP row set at step 0 whose feasibility mask is written directly."""
    from eam_rl4co_amd import ops

    B, M = mask.shape
    ost = oracle.State("tsp", np.zeros((B, M, 2), np.float32))
    ost.mask = np.ascontiguousarray(mask, dtype=np.uint8)
    st = ops.RolloutState("tsp", B, M, DEV)
    st.mask = t(mask != 0)
    return ost, st


def step(st, cache, mode, noise, top_k, top_p, **kw):
    from eam_rl4co_amd import ops

    a, lp, lps, lgs, status = ops.decode_step(st, cache, mode, noise=noise, clip=0.0, temp=1.0, want_logits=True,
                                              want_logprobs=True, top_k=top_k, top_p=top_p, **kw)
    assert int(status.item()) == 0
    return a.cpu().numpy(), lp.cpu().numpy(), lps.cpu().numpy(), lgs.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------
# the step kernel against the reference's verdicts
# ---------------------------------------------------------------------------------------------------------
def test_step_kernel_reproduces_the_recorded_verdicts_on_crafted_rows(oracle):
    g = torch.Generator().manual_seed(3)
    n = 0
    for i, c in enumerate(CASES):
        if not c["crafted"]:
            continue
        n += 1
        cache, mask = fc.crafted_cache(c, i)
        ost, st = tsp_states(oracle, mask)
        noise = torch.empty(1, c["x"].size).exponential_(1, generator=g)
        for planes in ((False, True) if c["x"].size >= 128 else (False,)):
            a, lp, lps, lgs = step(st, device_cache(cache, planes), "sampling", noise.to(DEV), c["top_k"], c["top_p"])
            assert np.array_equal(lgs[0], c["x"]), (c["name"], "the synthetic cache does not give the recorded row")
            keep = np.isfinite(lps[0])
            fc.check_keep(c, keep, "step kernel")
            fc.check_logp(lps[0], keep, c["x"], 1e-5, c["name"])
            assert keep[a[0]] and lp[0] == lps[0, a[0]]
            o = oracle.decode_step(ost, cache, "sampling", noise=noise.numpy(), clip=0.0, temp=1.0, num_heads=fc.H,
                                   want_all=True, top_k=c["top_k"], top_p=c["top_p"])
            assert_bits_equal(lps, o[3], f"{c['name']}: log-probs vs oracle")
            assert_bits_equal(a, o[0], f"{c['name']}: action vs oracle")
    assert n == len(mk.crafted())            # no crafted row is skipped


@pytest.mark.parametrize("M,planes", [(M, False) for M in fc.SIZES] + [(257, True)])
def test_step_kernel_agrees_with_the_restatement_on_its_own_logits(oracle, M, planes):
    """Random rows: the restatement is applied to the logits the kernel returned.  Rows whose running sum comes closer to
    the threshold than MARGIN_BOUND take no part in the keep-set comparison; at most 1 % may."""
    cache, mask = fc.random_cache(M, 1)
    ost, st = tsp_states(oracle, mask)
    dc = device_cache(cache, planes)
    B = mask.shape[0]
    noise = torch.empty(B, M).exponential_(1, generator=torch.Generator().manual_seed(M))
    rows = skipped = 0
    for p in fc.TOP_P:
        for k in fc.top_ks(M):
            a, lp, lps, lgs = step(st, dc, "sampling", noise.to(DEV), k, p)
            assert np.array_equal(np.isfinite(lgs), mask != 0)
            o = oracle.decode_step(ost, cache, "sampling", noise=noise.numpy(), clip=0.0, temp=1.0, num_heads=fc.H,
                                   want_all=True, top_k=k, top_p=p)
            assert_bits_equal(lps, o[3], f"log-probs vs oracle, top_k {k} top_p {p}")
            assert_bits_equal(a, o[0], "action vs oracle")
            for r in range(B):
                rows += 1
                keep, _, margin = fr.filter_row(lgs[r], k, p)
                got = np.isfinite(lps[r])
                assert got[a[r]] and lp[r] == lps[r, a[r]]
                if margin < mk.MARGIN_BOUND:
                    skipped += 1
                    continue
                assert np.array_equal(got, keep), (M, p, k, r, margin, np.flatnonzero(got != keep).tolist())
                fc.check_logp(lps[r], keep, lgs[r], 1e-5, (M, p, k, r))
    print(f"M {M}: rows {rows}, skipped by the margin rule {skipped}")
    assert skipped <= fc.MAX_SKIP_SHARE * rows


# ---------------------------------------------------------------------------------------------------------
# bit equality with the oracle on trained-shape policies at more than 64 nodes
# ---------------------------------------------------------------------------------------------------------
def _instance(env_name, N, B, seed):
    import eam_rl4co_amd as ea

    env = ea.get_env(env_name, generator_params=dict(num_loc=N), seed=seed)
    torch.manual_seed(seed)
    td_cpu = env.reset(batch_size=[B])
    return env, td_cpu, td_cpu["locs"].numpy(), instance_from_td(env_name, td_cpu)


@pytest.mark.parametrize("top_k,top_p", [(0, 0.8), (5, 0.0), (6, 0.9)])
@pytest.mark.parametrize("mode", ["greedy", "sampling"])
@pytest.mark.parametrize("env_name,N", [("tsp", 65), ("tsp", 101), ("tsp", 129), ("cvrp", 100)])
def test_filtered_steps_bit_equal_to_the_oracle_beyond_64_nodes(oracle, env_name, N, mode, top_k, top_p):
    from eam_rl4co_amd import ops
    from eam_rl4co_amd.policy import _env_step_, state_from_td

    B = 2
    cfg = "am_" + env_name
    pol = make_policy(cfg)
    env, td_cpu, locs, inst = _instance(env_name, N, B, 100 + N)
    td = td_cpu.to(DEV)
    sd = golden_weights(cfg)
    with torch.no_grad():
        emb, _ = pol.encoder(td)
        cache = pol.decoder._precompute_cache(emb)
    _, o_emb = oracle.encode(sd, env_name, locs, inst)
    oc = oracle.precompute(sd, env_name, o_emb, use_graph_context=pol.decoder.use_graph_context)
    ost = oracle.State(env_name, locs, inst)
    st = state_from_td(env_name, td, 0)
    M = ost.M
    g = torch.Generator().manual_seed(N)
    depot_masked = filtered = 0
    steps = 0
    while not ost.done.all():
        nz = torch.empty(B, M).exponential_(1, generator=g) if mode == "sampling" else None
        depot_masked += int((ost.mask[:, 0] == 0).any())
        oa, olp, _, ologp = oracle.decode_step(ost, oc, mode, noise=None if nz is None else nz.numpy(), want_all=True,
                                               top_k=top_k, top_p=top_p)
        a, lp, alls, _, status = ops.decode_step(st, cache, mode, noise=None if nz is None else nz.to(DEV),
                                                 want_logprobs=True, top_k=top_k, top_p=top_p)
        assert int(status.item()) == 0
        assert_bits_equal(alls, ologp, f"log-probs step {steps}")
        assert_bits_equal(a, oa, f"action step {steps}")
        assert_bits_equal(lp, olp, f"logp step {steps}")
        filtered += int((np.isneginf(ologp) & (ost.mask != 0)).any())
        ost.step(oa)
        _env_step_(st, a)
        assert_bits_equal(st.mask.to(torch.uint8), ost.mask, f"mask step {steps}")
        steps += 1
        assert steps <= 3 * M
    assert filtered >= 1, "the filter removes feasible nodes: the case tests it"
    if env_name == "cvrp":
        assert depot_masked >= 1


# ---------------------------------------------------------------------------------------------------------
# neutral settings
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [65, 129])
def test_neutral_settings_leave_the_step_unchanged(oracle, M):
    cache, mask = fc.random_cache(M, 2)
    _, st = tsp_states(oracle, mask)
    dc = device_cache(cache)
    noise = torch.empty(mask.shape[0], M).exponential_(1, generator=torch.Generator().manual_seed(M)).to(DEV)
    base = step(st, dc, "sampling", noise, 0, 0.0)
    for k, p in ((M, 0.0), (M + 7, 0.0), (0, 1.0), (0, 0.0), (M, 1.0)):
        got = step(st, dc, "sampling", noise, k, p)
        for x, y, what in zip(got, base, ("action", "logp", "log-probs", "logits")):
            assert_bits_equal(x, y, f"top_k {k} top_p {p}: {what}")
    # top_k = 1 leaves the largest entry alone: sampling then takes the greedy action with log-prob exactly 0
    greedy = step(st, dc, "greedy", None, 0, 0.0)
    one = step(st, dc, "sampling", noise, 1, 0.0)
    assert np.array_equal(one[0], greedy[0]) and (one[1] == 0.0).all()
    assert (np.isfinite(one[2]).sum(1) == 1).all()


def test_top_k_one_keeps_both_entries_of_a_tie_at_the_top(oracle):
    c = next(c for c in CASES if c["name"] == "topk1_tie_at_top")
    cache, mask = fc.crafted_cache(c, 0)
    _, st = tsp_states(oracle, mask)
    noise = torch.ones(1, c["x"].size).to(DEV)
    a, lp, lps, _ = step(st, device_cache(cache), "sampling", noise, 1, 0.0)
    assert np.isfinite(lps[0]).tolist() == [True, False, True, False]
    assert np.abs(lps[0, [0, 2]] + math.log(2.0)).max() <= 1e-6 and abs(lp[0] + math.log(2.0)) <= 1e-6


# ---------------------------------------------------------------------------------------------------------
# the streaming rollout kernel against a loop of fused steps
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_name,N,S,top_k,top_p", [("tsp", 65, 0, 0, 0.8), ("tsp", 129, 0, 6, 0.9), ("cvrp", 100, 0, 0, 0.8),
                                                     ("tsp", 65, 3, 5, 0.0), ("cvrp", 100, 2, 6, 0.9)])
def test_filtered_rollout_equals_the_step_loop(env_name, N, S, top_k, top_p):
    """ops.rollout with a filter runs the streaming kernel (the start-sharing and the register-resident kernels do not
    filter and must decline it, multistart included): actions and log-probs equal, bit for bit, a loop of
    decode_step(fuse_env_step=True); the seeded path equals the path fed with the tensor of the same draws."""
    from eam_rl4co_amd import ops
    from eam_rl4co_amd.policy import _env_step_, _max_decode_steps, state_from_td

    B = 2
    pol = make_policy("am_" + env_name)
    env, td_cpu, _, _ = _instance(env_name, N, B, 200 + N)
    td = td_cpu.to(DEV)
    with torch.no_grad():
        emb, _ = pol.encoder(td)
        cache = pol.decoder._precompute_cache(emb)
    M = td["locs"].shape[1]
    R = B * max(S, 1)
    t_max = _max_decode_steps(env_name, M, 1 if S else 0)

    def fresh():
        st = state_from_td(env_name, td, S)
        if S:       # select_start_nodes: row s * B + b starts at node s (TSP) / s + 1 (CVRP)
            start = torch.arange(S, device=DEV).repeat_interleave(B) + (0 if env_name == "tsp" else 1)
            _env_step_(st, start)
        return st

    seed = 20261018
    noise = ops.exp1_noise(seed, R, t_max, M, DEV)
    acts, lps, _, T, status = pol._rollout_stepwise(fresh(), cache, "sampling", noise, None, 10.0, 1.0, t_max, top_k, top_p)
    assert status == 0 and T > 0
    for how in ("tensor", "seeded"):
        kw = dict(noise=noise) if how == "tensor" else dict(seed=seed)
        a, lp, info = ops.rollout(fresh(), cache, "sampling", clip=10.0, temp=1.0, t_max=t_max, top_k=top_k, top_p=top_p, **kw)
        assert info.cpu().tolist() == [T, 0], how
        assert_bits_equal(a[:, :T], acts, f"{how}: actions")
        assert_bits_equal(lp[:, :T], lps, f"{how}: log-probs")
        assert torch.isfinite(lp).all()
    a0, lp0, _ = ops.rollout(fresh(), cache, "sampling", noise=noise, clip=10.0, temp=1.0, t_max=t_max)
    assert not torch.equal(lp0[:, :T], lps), "the filter changed nothing: the case does not test it"


# ---------------------------------------------------------------------------------------------------------
# the re-evaluation of filtered rollouts at more than 64 nodes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(top_p=0.8), dict(top_k=6, top_p=0.9)])
@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
def test_reevaluation_of_filtered_rollouts_at_100_nodes(env_name, kw, monkeypatch):
    """The value half of test_gradients_through_filtering_and_select_best at TSP-100 / CVRP-100: the re-evaluation's values
    equal the rollout's own per-step log-probs within 2e-5.  Then once more without the re-evaluation's "the chosen action
    always stays" line: the re-evaluation's own filter must keep every action the rollout chose -- a log-prob may become
    -inf only where a running sum is closer to the threshold than MARGIN_BOUND (the margin rule), in at most 1 % of the steps."""
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import train

    top_k, top_p = kw.get("top_k", 0), kw.get("top_p", 0.0)
    env = ea.get_env(env_name, generator_params=dict(num_loc=100), seed=8)
    torch.manual_seed(21)
    td = env.reset(batch_size=[3]).to(DEV)
    pol = make_policy("am_" + env_name).eval()
    torch.manual_seed(5)
    out = pol(td.clone(), env, phase="train", return_sum_log_likelihood=False, decode_type="sampling", **kw)
    lp, acts = out["log_likelihood"], out["actions"]
    assert lp.requires_grad and torch.isfinite(lp).all()

    def reeval():
        return train.evaluate_log_likelihood(pol, td, env, acts, num_starts=0, multistart=False, top_k=top_k, top_p=top_p,
                                             native=False)

    re = reeval()
    assert torch.isfinite(re).all()
    np.testing.assert_allclose(re.detach().cpu().numpy(), lp.detach().cpu().numpy(), rtol=0, atol=2e-5)

    seen = []
    filt, scatter_ = train._filter_logits_, torch.Tensor.scatter_
    monkeypatch.setattr(train, "_filter_logits_", lambda logits, *a: (seen.append(logits.detach()), filt(logits, *a))[1])
    # `drop.scatter_(-1, act[..., None], False)` is the only scatter_ of a Python bool: without it nothing protects the action
    monkeypatch.setattr(torch.Tensor, "scatter_",
                        lambda self, dim, index, src=None, **k: self if src is False else scatter_(self, dim, index, src, **k))
    bare = reeval().detach()
    monkeypatch.undo()
    assert len(seen) >= 1
    x = torch.cat(seen, 0).cpu().numpy()
    assert x.shape[:2] == tuple(bare.shape), "one call per chunk of rows"
    lost = torch.nonzero(~torch.isfinite(bare)).cpu().tolist()
    for r, s in lost:
        margin = fr.filter_row(x[r, s], top_k, top_p)[2]
        assert margin < mk.MARGIN_BOUND, (r, s, margin)
    print(f"{env_name} {kw}: steps {bare.numel()}, lost to the margin rule {len(lost)}")
    assert len(lost) <= fc.MAX_SKIP_SHARE * bare.numel()
    ok = torch.isfinite(bare)
    np.testing.assert_allclose(bare[ok].cpu().numpy(), lp.detach()[ok].cpu().numpy(), rtol=0, atol=2e-5)
