"""GPU: the decode arithmetic of the three whole-rollout kernels (`ms_mfma`, `resident`, `stream`) and of the per-step kernel
behind ops.decode_step against the float64 restatement (tests/rollout_ref.py), on synthetic decoder caches at the scales of
a trained policy (tests/rollout_cases.py): query assembly with the state columns, the masked 8-head glimpse, logits, tanh clip,
temperature, log-softmax and the greedy / sampling selection.  The env rule itself is tests/test_gpu_step_rule.py's.

Per case, mode and kernel (the kernel forced with test_gpu_step_rule.forced, wherever test_gpu_step_rule.supported admits it):
  rollout      status 0, every action feasible and every row finished by step_ref's replay, nothing written after the last step
  log-probs    logps[r, t] within the case's bound of the float64 log-prob of the kernel's own action; exactly 0 on finished rows
  selection    the float64 key of the chosen node within twice that bound of the float64 maximum over the feasible nodes
  tie rule     `tie` cases: the lower twin of every pair precedes the higher one in every row's tour (both stay equally feasible
               with bit-identical keys until one is taken, so every row decides every pair once) -- greedy and sampling
  saturation   greedy, clip > 0: where a feasible node has u64 >= 9.5 (d_tanhf is exactly 1 above 9) the chosen index is at most
               the lowest such index; in a `saturated` case at least a quarter of the live steps are such steps
  agreement    every kernel that runs the case returns the same actions and log-probs, bit for bit
  per step     ops.decode_step(mode="evaluate", fuse_env_step=True, want_logprobs=True) along that trajectory, slot-major and
               plane-major: the full log-prob vector within its own bound at the feasible entries, exactly -inf elsewhere, the selected
               log-prob bit-equal to the rollout's
The twin pairs sit where the kernels' selection code changes: (1, 2) one lane quad of the MFMA kernel, (3, 4) neighbouring quads,
(31, 32) a mask word, (63, 64) the resident kernel's two blocks, (5, 69) one lane of the resident kernel, and the last two nodes.
The bounds are rollout_cases.check's; none comes from the kernels.
"""
import numpy as np
import pytest
import torch

import rollout_cases as rc
import step_ref
import test_gpu_step_rule as sr
from test_gpu_parity import DEV, assert_bits_equal

pytestmark = pytest.mark.gpu

FIGURES = {}                # (case, mode, kernel) -> figures of rollout_cases.check of the cases that ran in this process


def device_cache(c, cch, planes):
    """ops.DecodeCache of the synthetic cache: slot-major [B, M, slots * E] or plane-major [slots, B, M, E]."""
    from eam_rl4co_amd import ops

    env = c["env"]
    parts = dict(cch, L=torch.zeros_like(cch["K"]))               # (the unfolded logit key: no kernel reads it)
    rows = [parts[n] for n in ops.slot_map(env)]
    buf = torch.stack(rows) if planes else torch.cat(rows, -1)
    dev = lambda x: None if x is None else x.to(DEV).contiguous()
    cvec = None if cch["Cvec"] is None else cch["Cvec"].reshape(-1)
    return ops.DecodeCache(env, dev(buf), dev(cvec), dev(cch["gctx"]), None, sr.H, dyn=dev(cch["dyn"]), embed_dim=rc.E)


def kernels_of(c):
    return [k for k in sr.KERNELS if sr.supported(k, c["env"], c["M"], c["S"])]


# which kernels run a case of M nodes and S starts (M = ms_mfma, R = resident, S = stream); PDP never runs on ms_mfma
EXPECTED_KERNELS = {
    (2, 1): "RS", (2, 4): "MRS", (2, 17): "MRS", (20, 1): "RS", (20, 4): "MRS", (20, 17): "MRS", (21, 1): "RS", (21, 4): "MRS",
    (21, 17): "MRS", (33, 1): "RS", (33, 4): "MRS", (33, 17): "MRS", (65, 1): "RS", (65, 4): "MRS", (65, 17): "MRS",
    (100, 1): "RS", (100, 4): "MRS", (100, 17): "MRS", (112, 1): "RS", (112, 4): "MRS", (112, 17): "MRS",
    (113, 1): "RS", (113, 4): "RS", (113, 17): "RS", (128, 1): "RS", (128, 4): "RS", (128, 17): "RS",
    (129, 1): "S", (129, 4): "S", (129, 17): "S"}
EXPECTED_KERNELS_PDP = {(21, 1): "RS", (21, 4): "RS", (65, 1): "RS", (65, 4): "RS"}


def test_kernel_combinations_are_the_expected_ones():
    """No kernel silently drops out: what runs per (env, M, S), against an explicit table."""
    letter = {"M": "ms_mfma", "R": "resident", "S": "stream"}
    for c in rc.CASES.values():
        table = EXPECTED_KERNELS_PDP if c["env"] == "pdp" else EXPECTED_KERNELS
        assert kernels_of(c) == [letter[x] for x in table[(c["M"], c["S"])]], c["name"]
    assert {(c["M"], c["S"]) for c in rc.CASES.values() if c["env"] != "pdp"} == set(EXPECTED_KERNELS)


def run_rollout(c, states, cache, kernel, mode, clip, temp, noise):
    from eam_rl4co_amd import ops

    st = sr.upload(c, states)
    T = rc.t_max(c)
    with sr.forced(kernel):
        assert ops.rollout_kernel(st, cache, st.R, T) == kernel, f"{c['name']}: {kernel} is not the kernel that runs"
        kw = dict(noise=noise) if mode == "sampling" else {}
        actions, logps, info = ops.rollout(st, cache, mode=mode, t_max=T, clip=clip, temp=temp, **kw)
        info = info.cpu().numpy()
    steps, status = int(info[0]), int(info[1])
    assert status == 0, f"{c['name']} {mode} on {kernel}: status {status}"
    assert 0 < steps <= T
    actions, logps = actions.cpu(), logps.cpu()
    assert not actions[:, steps:].any() and not logps[:, steps:].any(), "something was written after the last step"
    return actions[:, :steps].contiguous(), logps[:, :steps].contiguous()


def check_decode_step(c, cch, states, actions, logps, res, clip, temp, planes):
    from eam_rl4co_amd import ops

    st = sr.upload(c, states)
    cache = device_cache(c, cch, planes)
    given = actions.T.contiguous().to(DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    lp, lps = [], []
    for k in range(actions.shape[1]):
        _, a, b, _, _ = ops.decode_step(st, cache, mode="evaluate", given=given[k], clip=clip, temp=temp, fuse_env_step=True,
                                        want_logprobs=True, status=status)
        lp.append(a)
        lps.append(b)
    assert int(status.item()) == 0
    lp, lps = torch.stack(lp, 1).cpu(), torch.stack(lps, 1).cpu()
    what = f"{c['name']} decode_step {'plane' if planes else 'slot'}-major"
    mask, want, live = res["op"]["mask"], res["r64"]["logp_all"], ~res["op"]["done"]
    assert bool((lps[~mask] == -np.inf).all()), f"{what}: an infeasible entry is not -inf"
    err = float((lps.double() - want)[mask].abs().max())
    bound = res["figures"]["bound_full"]
    print(f"{what}: full vector {err:.3e} of {bound:.3e}")
    assert err <= bound, f"{what}: full log-prob vector {err:.3e} from float64, bound {bound:.3e}"
    assert_bits_equal(lp[live].numpy(), logps[live].numpy(), f"{what}: selected log-prob vs the rollout's")
    assert bool((lp[~live] == 0).all())


@pytest.mark.parametrize("name", rc.NAMES)
def test_rollout_arithmetic(name):
    c, batch, cch, q = rc.operands(name)
    clip, temp = rc.clip_temp(c)
    states = step_ref.reset_rows(batch, c["S"])
    cache = device_cache(c, cch, planes=c["M"] > 128)
    noise = q.to(DEV)
    for mode in rc.MODES:
        runs = {k: run_rollout(c, states, cache, k, mode, clip, temp, noise) for k in kernels_of(c)}
        res = {}
        for k, (actions, logps) in runs.items():
            same = [j for j in res if torch.equal(runs[j][0], actions) and
                    np.array_equal(runs[j][1].numpy().view(np.uint32), logps.numpy().view(np.uint32))]
            res[k] = res[same[0]] if same else rc.check(name, mode, actions, logps)       # (one float64 run per distinct result)
            f = res[k]["figures"]
            print(f"{name} {mode} {k}: " + ", ".join(f"{a} {b:.3e}" for a, b in f.items()))
            FIGURES[(name, mode, k)] = f
        for k in runs:
            assert res[k]["misses"] == [], f"{name} {mode} on {k}"
        first = next(iter(runs))
        for k in runs:
            assert torch.equal(runs[k][0], runs[first][0]), f"{name} {mode}: the actions of {k} and {first} differ"
            assert_bits_equal(runs[k][1].numpy(), runs[first][1].numpy(), f"{name} {mode}: log-probs of {k} vs {first}")
        k = "resident" if "resident" in runs else "stream"
        for planes in (False, True):
            check_decode_step(c, cch, states, *runs[k], res[k], clip, temp, planes)


def test_seeded_sampling_equals_the_noise_tensor_path():
    """ops.rollout(seed=...) on the start-sharing kernel (draws computed in place) == the same call fed ops.exp1_noise of that
    seed, bit for bit, at the peaked scale."""
    from eam_rl4co_amd import ops

    name = "tsp_peaked_M20_S4"
    c, batch, cch, _ = rc.operands(name)
    states = step_ref.reset_rows(batch, c["S"])
    cache = device_cache(c, cch, planes=False)
    T, seed = rc.t_max(c), 20240229
    out = []
    for kw in (dict(seed=seed), dict(noise=ops.exp1_noise(seed, len(states), T, c["M"], DEV))):
        st = sr.upload(c, states)
        with sr.forced("ms_mfma"):
            assert ops.rollout_kernel(st, cache, st.R, T) == "ms_mfma"
            actions, logps, info = ops.rollout(st, cache, mode="sampling", t_max=T, **kw)
        assert int(info[1]) == 0
        out.append((actions.cpu(), logps.cpu()))
    assert torch.equal(out[0][0], out[1][0])
    assert_bits_equal(out[0][1].numpy(), out[1][1].numpy(), "seeded vs noise tensor: log-probs")
    assert rc.check(name, "sampling", *out[0], noise=ops.exp1_noise(seed, len(states), T, c["M"], DEV).cpu())["misses"] == []


def test_report_the_measured_errors():
    """Per kind: the worst measured log-prob error over its bound among the cases that ran before it in this process (a report,
    shown with -s / -rA; it asserts nothing and is empty when run alone)."""
    worst = {}
    for (name, mode, k), f in FIGURES.items():
        kind = rc.CASES[name]["kind"]
        ratio = f["err"] / f["bound"] if f.get("bound") else 0.0
        if "err" in f and ratio >= worst.get(kind, (-1.0,))[0]:
            worst[kind] = (ratio, name, mode, k, f["err"], f["bound"], f["err32"])
    for kind, w in worst.items():
        print(f"{kind}: worst error / bound {w[0]:.3f} ({w[1]} {w[2]} {w[3]}: {w[4]:.3e} of {w[5]:.3e}; float32 restatement {w[6]:.3e})")
