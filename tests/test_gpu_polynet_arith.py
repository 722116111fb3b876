"""GPU: the decode arithmetic of the PolyNet case of the start-sharing rollout kernel (k_rollout_ms_mfma<..., PolyArgs>, reached with
ops.rollout(..., poly=)) against the float64 restatement of the PolyNet pointer (tests/rollout_ref.py, `poly`), on the synthetic
caches and weights of tests/polynet_cases.py: the fixed-chunk glimpse of every key-tile count, the three streamed weight GEMMs,
the ReLU, the strategy lookup, the query-tile split and the split of more than 128 rows per instance into launches.

Per case and mode (greedy, sampling from the case's noise tensor):
  rollout       status 0, every action feasible and every row finished by step_ref's replay, nothing written after `steps`
  log-probs     within the case's bound of the float64 log-prob of the kernel's own action; exactly 0 on finished rows
  selection     the float64 key of the chosen node within twice that bound of the float64 maximum; the twins' order in `tie`
                cases, the lowest saturated index in greedy rollouts (polynet_cases.check = rollout_cases.check)
  final state   cur, used, mask, visited, done (first, istep) after the call == step_ref's replay of the returned actions over
                `steps` steps, finished CVRP rows stepped with the depot
  evaluate      mode="evaluate" on the greedy rollout's actions returns them with bit-identical log-probs
On one case per key-tile count and env: slot-major and plane-major caches give the same actions and log-probs bit for bit; there
and on both cases of more than 128 rows per instance: ops.rollout(seed=) == the same call fed ops.exp1_noise of that seed.
The bounds are polynet_cases'; none comes from the kernel.  Every figure is printed before it is asserted.
"""
import numpy as np
import pytest
import torch

import polynet_cases as pc
import rollout_cases as rc
import step_ref
import test_gpu_step_rule as sr
from test_gpu_parity import DEV, assert_bits_equal

pytestmark = pytest.mark.gpu

FIGURES = {}                # (case, mode) -> figures of polynet_cases.check of the cases that ran in this process


# What the launcher does with a case (launch_env_t, launch_t and rollout_call): (M, S, B) -> (key tiles RTT, workgroups per
# instance nsplit = min(256 // B, query tiles) of every launch, launches = ceil(S / 128)).
EXPECTED_LAUNCHES = {
    (2, 2, 3): (2, (1,)), (2, 17, 3): (2, (2,)), (20, 17, 3): (2, (2,)), (20, 16, 3): (2, (1,)), (31, 16, 3): (2, (1,)),
    (31, 17, 3): (2, (2,)), (32, 17, 3): (2, (2,)), (32, 2, 3): (2, (1,)), (32, 16, 3): (2, (1,)), (33, 4, 3): (4, (1,)),
    (33, 17, 3): (4, (2,)), (33, 2, 3): (4, (1,)), (63, 17, 3): (4, (2,)), (63, 16, 3): (4, (1,)), (64, 16, 3): (4, (1,)),
    (64, 2, 3): (4, (1,)), (64, 17, 3): (4, (2,)), (65, 2, 3): (7, (1,)), (65, 17, 3): (7, (2,)), (65, 4, 3): (7, (1,)),
    (100, 2, 3): (7, (1,)), (100, 4, 3): (7, (1,)), (112, 17, 3): (7, (2,)), (112, 2, 3): (7, (1,)), (112, 16, 3): (7, (1,)),
    (21, 17, 3): (2, (2,)), (21, 16, 3): (2, (1,)),
    (20, 40, 100): (2, (2,)), (20, 17, 129): (2, (1,)), (20, 128, 1): (2, (8,)), (20, 130, 3): (2, (8, 1)),
    (21, 128, 1): (2, (8,)), (21, 130, 3): (2, (8, 1))}


def launches_of(M, S, B):
    """The launcher's rule, restated: -> (RTT, nsplit of every launch)."""
    tiles = lambda s: -(-s // 16)
    return (2 if M <= 32 else 4 if M <= 64 else 7,
            tuple(max(1, min(256 // B, tiles(min(128, S - s0)))) for s0 in range(0, S, 128)))


def test_case_set_reaches_every_launch_path():
    """No path silently drops out of the table: what every case launches, against an explicit table, and the paths the set must
    reach -- all three key-tile counts for both envs, nsplit 1 with several tiles looped, 2 over an odd tile count, 8, and two
    launches for both envs."""
    cases = list(pc.CASES.values())
    for c in cases:
        assert EXPECTED_LAUNCHES[(c["M"], c["S"], c["B"])] == launches_of(c["M"], c["S"], c["B"]), c["name"]
    assert {(c["M"], c["S"], c["B"]) for c in cases} == set(EXPECTED_LAUNCHES)
    paths = {(c["env"],) + EXPECTED_LAUNCHES[(c["M"], c["S"], c["B"])] + (-(-min(c["S"], 128) // 16),) for c in cases}
    for env in ("tsp", "cvrp"):
        assert {p[1] for p in paths if p[0] == env} == {2, 4, 7}
        assert any(len(p[2]) == 2 for p in paths if p[0] == env)                        # two launches
        assert any(p[2][0] == 8 for p in paths if p[0] == env)
    assert any(p[2] == (1,) and p[3] == 2 for p in paths)                               # tiles looped in one workgroup
    assert any(p[2] == (2,) and p[3] == 3 for p in paths)                               # 3 tiles over 2 workgroups
    for n in pc.PER_TILE_COUNT + pc.SPLIT:
        c = pc.CASES[n]
        print(f"{n}: RTT, nsplit per launch = {launches_of(c['M'], c['S'], c['B'])}")


def device_cache(c, cch, planes=False):
    """ops.DecodeCache of the case's cache, the unfolded logit key included: slot-major [B, M, slots * E] or plane-major."""
    from eam_rl4co_amd import ops

    rows = [cch[n] for n in ops.slot_map(c["env"])]
    buf = torch.stack(rows) if planes else torch.cat(rows, -1)
    dev = lambda x: None if x is None else x.to(DEV).contiguous()
    return ops.DecodeCache(c["env"], dev(buf), dev(cch["Cvec"].reshape(-1)), dev(cch["gctx"]), None, sr.H, embed_dim=pc.E)


def run_rollout(c, states, cache, poly, mode, **kw):
    """One ops.rollout(poly=) -> (actions [R, steps], logps [R, steps], the state object after the call)."""
    from eam_rl4co_amd import ops

    st = sr.upload(c, states, B=c["B"])
    clip, temp = pc.clip_temp(c)
    T = pc.t_max(c)
    assert ops.rollout_polynet_supported(c["env"], cache, st.R)
    actions, logps, info = ops.rollout(st, cache, mode=mode, t_max=T, clip=clip, temp=temp, poly=poly, **kw)
    steps, status = (int(x) for x in info.cpu().numpy())
    assert status == 0, f"{c['name']} {mode}: status {status}"
    assert 0 < steps <= T
    actions, logps = actions.cpu(), logps.cpu()
    assert not actions[:, steps:].any() and not logps[:, steps:].any(), "something was written after the last step"
    return actions[:, :steps].contiguous(), logps[:, :steps].contiguous(), st


def assert_final_state(c, batch, actions, st, what):
    """The state tensors after the call against step_ref's replay of the returned actions (all `steps` columns: a finished CVRP
    row is stepped with the depot, as the reference's loop does)."""
    final = step_ref.replay(batch, actions.numpy(), c["S"])[-1]
    assert all(bool(s["done"]) for s in final), f"{what}: rows are left unfinished"
    sr.assert_state_equal(sr.device_slots(st), sr.expected_slots(c, final), f"{what}: final state")


@pytest.mark.parametrize("name", pc.NAMES)
def test_polynet_rollout_arithmetic(name):
    c, batch, cch, q = pc.operands(name)
    states = step_ref.reset_rows(batch, c["S"])
    cache, poly = device_cache(c, cch), pc.polynet_operands(c, cch, DEV)
    noise = q.to(DEV)
    runs = {mode: run_rollout(c, states, cache, poly, mode, **(dict(noise=noise) if mode == "sampling" else {})) for mode in pc.MODES}
    res = {}
    for mode, (actions, logps, st) in runs.items():
        res[mode] = pc.check(name, mode, actions, logps)
        f = res[mode]["figures"]
        print(f"{name} {mode}: " + ", ".join(f"{a} {b:.3e}" for a, b in f.items()) + f"; launches {launches_of(c['M'], c['S'], c['B'])}")
        FIGURES[(name, mode)] = f
    for mode, (actions, logps, st) in runs.items():
        assert res[mode]["misses"] == [], f"{name} {mode}"
        assert_final_state(c, batch, actions, st, f"{name} {mode}")
    # evaluate == greedy
    actions, logps, _ = runs["greedy"]
    a2, l2, st2 = run_rollout(c, states, cache, poly, "evaluate", given=actions.to(DEV))
    assert torch.equal(a2, actions), f"{name}: evaluate returns other actions than it was given"
    assert_bits_equal(l2.numpy(), logps.numpy(), f"{name}: evaluate vs greedy log-probs")
    assert_final_state(c, batch, a2, st2, f"{name} evaluate")


@pytest.mark.parametrize("name", pc.PER_TILE_COUNT)
def test_both_cache_layouts_give_the_same_rollout(name):
    c, batch, cch, q = pc.operands(name)
    states = step_ref.reset_rows(batch, c["S"])
    poly = pc.polynet_operands(c, cch, DEV)
    noise = q.to(DEV)
    for mode in pc.MODES:
        kw = dict(noise=noise) if mode == "sampling" else {}
        slot, plane = (run_rollout(c, states, device_cache(c, cch, planes), poly, mode, **kw) for planes in (False, True))
        same = torch.equal(slot[0], plane[0])
        err = float((slot[1].double() - plane[1].double()).abs().max()) if slot[1].shape == plane[1].shape else float("nan")
        print(f"{name} {mode}: plane-major against slot-major: actions equal {same}, log-probs {err:.3e} apart")
        assert same, f"{name} {mode}: the actions of the two cache layouts differ"
        assert_bits_equal(plane[1].numpy(), slot[1].numpy(), f"{name} {mode}: log-probs, plane-major vs slot-major")
        assert pc.check(name, mode, plane[0], plane[1])["misses"] == []


@pytest.mark.parametrize("name", pc.PER_TILE_COUNT + pc.SPLIT)
def test_seeded_sampling_equals_the_noise_tensor_path(name):
    from eam_rl4co_amd import ops

    c, batch, cch, _ = pc.operands(name)
    states = step_ref.reset_rows(batch, c["S"])
    cache, poly = device_cache(c, cch), pc.polynet_operands(c, cch, DEV)
    seed = 20240229
    tensor = ops.exp1_noise(seed, len(states), pc.t_max(c), c["M"], DEV)
    seeded = run_rollout(c, states, cache, poly, "sampling", seed=seed)
    fed = run_rollout(c, states, cache, poly, "sampling", noise=tensor)
    assert torch.equal(seeded[0], fed[0]), f"{name}: seeded and fed rollouts differ"
    assert_bits_equal(seeded[1].numpy(), fed[1].numpy(), f"{name}: seeded vs noise tensor: log-probs")
    res = pc.check(name, "sampling", seeded[0], seeded[1], noise=tensor.cpu())
    print(f"{name} seeded: " + ", ".join(f"{a} {b:.3e}" for a, b in res["figures"].items()))
    assert res["misses"] == []
    assert_final_state(c, batch, seeded[0], seeded[2], f"{name} seeded")


def test_limits():
    from eam_rl4co_amd import ops

    def case(env, M, S):
        c = dict(pc.CASES["tsp_normal_M20_S16_B3_k16" if env == "tsp" else "cvrp_normal_M21_S16_B3_k16"], M=M, S=S, env=env)
        nslot = len(ops.slot_map(env))
        cache = ops.DecodeCache(env, torch.zeros(3, M, nslot * pc.E, device=DEV), torch.zeros(pc.E, device=DEV), torch.zeros(3, pc.E, device=DEV),
                                None, sr.H, dyn=torch.zeros(3, pc.E, device=DEV) if env == "sdvrp" else None, embed_dim=pc.E)
        return c, cache

    for M in (2, 112):
        c, cache = case("tsp", M, 2)
        assert ops.rollout_polynet_supported("tsp", cache, 2 * 3)
    _, _, cch, _ = pc.operands("tsp_normal_M20_S16_B3_k16")
    poly = pc.polynet_operands(None, cch, DEV)
    for env, M, S in (("tsp", 113, 2), ("tsp", 20, 1), ("sdvrp", 21, 2)):
        c, cache = case(env, M, S)
        assert not ops.rollout_polynet_supported(env, cache, S * 3), (env, M, S)
        st = sr.upload(c, step_ref.reset_rows(rc.instances(c), S))
        with pytest.raises(NotImplementedError):
            ops.rollout(st, cache, poly=poly)


def test_report_the_measured_errors():
    """Per kind: the worst measured log-prob error over its bound among the cases that ran before it in this process (a report,
    shown with -s / -rA; it asserts nothing and is empty when run alone)."""
    worst = {}
    for (name, mode), f in FIGURES.items():
        kind = pc.CASES[name]["kind"]
        ratio = f["err"] / f["bound"] if f.get("bound") else 0.0
        if "err" in f and ratio >= worst.get(kind, (-1.0,))[0]:
            worst[kind] = (ratio, name, mode, f["err"], f["bound"], f["err32"])
    for kind, w in worst.items():
        print(f"{kind}: worst error / bound {w[0]:.3f} ({w[1]} {w[2]}: {w[3]:.3e} of {w[4]:.3e}; float32 restatement {w[5]:.3e})")
