"""GPU: the five device restatements of every env's step-and-mask rule against tests/step_ref.py, on the boundary cases of
tests/step_cases.py (rows that sit ON a comparison of the rule) and their padded variants.

  (a) the stand-alone step kernels (`ops.*_step_mask_`, `cvrp_mask_`)            csrc/env_reward.hip, csrc/pdp.hip
  (b) the state replay of the re-evaluation (`ops.replay_states[_sdvrp]`)        csrc/env_reward.hip
  (c) the per-step decode kernel with the fused env step (`ops.decode_step`)      csrc/decode_step.hip
  (d) the three whole-rollout kernels, forced in turn (`ops.rollout`)            rollout_multistart / rollout_resident / decode_step
  (e) the same, teacher-forced through the boundary (`mode="evaluate"`)
  (f) the same, started from a mid-episode state

Everything is compared exactly: masks, `done`, integer state, float32 state bit for bit.  (c)-(f) run on an ALL-ZERO decoder
cache: every feasible logit is then 0, the kernels' arithmetic drops out and only the rule is left -- log p = -log(number of
feasible nodes), and with noise[r, t, n] = (1 + rank of n in the row's preference list) / M the sampling key exp(lp) / noise
picks the first feasible node of the list, which is step_ref.rollout_first_feasible.  The one tolerance: exp(-logp) is within
0.25 of the reference's feasible count -- counts are integers <= 129, so neighbouring counts are 1 apart.
"""
import functools

import numpy as np
import pytest
import torch

import step_cases
import step_ref
from eam_rl4co_amd import env_spec
from test_gpu_parity import DEV, assert_bits_equal, t

pytestmark = pytest.mark.gpu

E, H = 128, 8               # the embedding width and head count the rollout kernels are built for
NAMES = step_cases.NAMES
EXERCISED = {}              # test -> what ran, printed by test_report_what_was_exercised


def note(test, what):
    EXERCISED.setdefault(test, []).append(what)


# ---------------------------------------------------------------------------------------------------------------------
# references (computed once per case, size and number of starts; read-only)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name, M=None, S=1):
    """-> dict(case, prefs [R, T, M], actions [R, T'], counts [R, T'], hist = states after reset and after every step)."""
    case = step_cases.case_by_name(name)
    if M is not None:
        case = step_cases.padded(case, M)
    prefs = step_cases.prefs(case, S)
    actions, counts, final, masks = step_ref.rollout_first_feasible(case["batch"], prefs)
    hist = step_ref.replay(case["batch"], actions, S)
    return {"case": case, "prefs": prefs, "actions": actions, "counts": counts, "hist": hist, "S": S}


def sizes_for(name, big=False):
    """(M or None for the named size, S) of a case: the named case with 1 and 4 starts, the padded ones with 4."""
    env = step_cases.case_by_name(name)["env"]
    out = [(None, 1), (None, 4)] + [(M, 4) for M in step_cases.PADDED_M if not (env == "pdp" and M % 2 == 0)]
    if big and env in ("tsp", "cvrp"):
        out.append((step_cases.BIG_M, 4))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# step_ref states <-> ops.RolloutState
# ---------------------------------------------------------------------------------------------------------------------
def row_slots(env_name):
    return [f for f in env_spec.spec(env_name).fields if f.per_row]


def upload(case, states, B=3):
    """ops.RolloutState holding the step_ref states (row r: instance r % B), per-instance tensors included."""
    from eam_rl4co_amd import ops

    env = env_spec.spec(case["env"]).name
    R, M = len(states), case["M"]
    st = ops.RolloutState(env, R, M, DEV)
    st.mask = t(np.stack([s["mask"] for s in states]))
    st.done = t(np.array([s["done"] for s in states]))
    for f in env_spec.ENV_SPECS[env].fields:
        rows = states if f.per_row else states[:B]
        v = np.stack([np.asarray(s[f.slot]) for s in rows])
        dtype = torch.uint8 if f.dtype == torch.bool else f.dtype
        setattr(st, f.slot, t(v).to(dtype).contiguous())
    return st


def expected_slots(case, states):
    env = env_spec.spec(case["env"]).name
    out = {"mask": np.stack([s["mask"] for s in states]), "done": np.array([s["done"] for s in states])}
    for f in row_slots(env):
        v = np.stack([np.asarray(s[f.slot]) for s in states])
        out[f.slot] = v.astype({torch.float32: np.float32, torch.int64: np.int64}.get(f.dtype, np.uint8))
    return out


def device_slots(st):
    out = {"mask": st.mask, "done": st.done}
    for f in row_slots(st.env_name):
        out[f.slot] = getattr(st, f.slot)
    return {k: v.clone() for k, v in out.items()}


def assert_state_equal(got, want, what):
    """got: {slot: device tensor or array}, want: {slot: array}; bool planes compare as 0 / 1."""
    assert set(got) == set(want)
    for k in want:
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else np.asarray(got[k])
        w = want[k]
        if g.dtype == np.bool_ or w.dtype == np.bool_:
            g, w = g.astype(np.uint8), w.astype(np.uint8)
        assert_bits_equal(g.reshape(w.shape), w, f"{what}: {k}")


def stacked(snapshots):
    return {k: torch.stack([s[k] for s in snapshots]) for k in snapshots[0]}


def stacked_expected(case, hist):
    per = [expected_slots(case, states) for states in hist]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def zero_cache(case, planes=False):
    from eam_rl4co_amd import ops

    env = env_spec.spec(case["env"]).name
    B, M = 3, case["M"]
    nslot = len(ops.slot_map(env))
    buf = torch.zeros((nslot, B, M, E) if planes else (B, M, nslot * E), device=DEV)
    ncol = env_spec.ENV_SPECS[env].n_state_cols
    cvec = None if env == "pdp" else torch.zeros(max(ncol, 1) * E, device=DEV)
    dyn = torch.zeros(3, E, device=DEV) if env == "sdvrp" else None
    return ops.DecodeCache(env, buf, cvec, torch.zeros(B, E, device=DEV), None, H, dyn=dyn, embed_dim=E)


# ---------------------------------------------------------------------------------------------------------------------
# (a) stand-alone step kernels
# ---------------------------------------------------------------------------------------------------------------------
def step_args(st, entry, action):
    return [action if a == env_spec.ACTION else None if a is None else getattr(st, a) for a in entry]


@pytest.mark.parametrize("name", NAMES)
def test_step_kernels_follow_the_rule(name):
    """ops.<step>_ after every scripted action: mask, done and every state slot equal step_ref's; cvrp_mask_ (mask only) too."""
    from eam_rl4co_amd import ops

    for M, S in sizes_for(name, big=True):
        ref = reference(name, M, S)
        case, hist, actions = ref["case"], ref["hist"], ref["actions"]
        env = env_spec.spec(case["env"]).name
        fn, entry = env_spec.ENV_SPECS[env].step
        st = upload(case, hist[0])
        acts = t(actions.T.copy())
        snaps, mask_only = [device_slots(st)], []
        for k in range(actions.shape[1]):
            getattr(ops, fn)(*step_args(st, entry, acts[k]))
            snaps.append(device_slots(st))
            if env == "cvrp":
                m = torch.zeros_like(st.mask)
                ops.cvrp_mask_(st.visited, st.used, st.vcap, st.demand, st.cur, m)
                mask_only.append(m)
        assert_state_equal(stacked(snaps), stacked_expected(case, hist), f"{case['name']} S={S}")
        if mask_only:
            assert_bits_equal(torch.stack(mask_only), stacked_expected(case, hist[1:])["mask"], "cvrp_mask_")
        note("step kernels", f"{case['name']} S={S} T={actions.shape[1]}")


# ---------------------------------------------------------------------------------------------------------------------
# (b) replay kernels
# ---------------------------------------------------------------------------------------------------------------------
def unpack_bits(bits, M):
    """[R, T, 4] (bit n = node n) or [R, T, nkc, 4] (bit i of chunk c = node 112 c + i) int32 -> bool [R, T, M]."""
    w = bits.cpu().numpy().view(np.uint32)
    b = ((w[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)
    b = b.reshape(w.shape[:-1] + (128,))
    if w.ndim == 3:
        return b[..., :M]
    return b[..., :112].reshape(w.shape[0], w.shape[1], -1)[..., :M]


@pytest.mark.parametrize("name", [n for n in NAMES if step_cases.case_by_name(n)["env"] not in ("tsp", "pdp")])
def test_replay_kernels_follow_the_rule(name):
    """replay_states / replay_states_sdvrp: the mask, current node and state columns BEFORE every step of the script, in the
    one-chunk layout (M <= 112) and the chunked one."""
    from eam_rl4co_amd import ops

    for M, S in sizes_for(name, big=True):
        ref = reference(name, M, S)
        case, hist, actions = ref["case"], ref["hist"], ref["actions"]
        env = env_spec.spec(case["env"]).name
        R, T = actions.shape
        st = upload(case, hist[0])
        before = device_slots(st)
        if env == "sdvrp":
            bits, idxA, sc, rem = ops.replay_states_sdvrp(st, t(actions))
        else:
            bits, idxA, sc = ops.replay_states(st, t(actions), 3)
        assert bits.dim() == (4 if case["M"] > 112 else 3)
        want = stacked_expected(case, hist[:T])
        assert_bits_equal(unpack_bits(bits, case["M"]), want["mask"].transpose(1, 0, 2), f"{case['name']}: mask bits")
        assert_bits_equal(idxA, want["cur"].T.astype(np.int32), f"{case['name']}: idxA")
        free = (want["vcap"] - want["used"]).astype(np.float32)         # one float32 subtraction
        if env == "pctsp":
            free = np.where(free < 0, np.float32(0), free)
        assert_bits_equal(sc[0], free.T.copy(), f"{case['name']}: state column 0")
        if env == "cvrptw":
            assert_bits_equal(sc[1], want["time"].T.copy(), f"{case['name']}: clock column")
        if env == "sdvrp":
            r = rem.cpu().numpy()
            if r.ndim == 4:
                r = r[..., :112].reshape(R, T, -1)
            assert_bits_equal(r[..., :case["M"]], want["rem"].transpose(1, 0, 2), f"{case['name']}: rem")
            assert not r[..., case["M"]:].any()
        assert_state_equal(device_slots(st), {k: v.cpu().numpy() for k, v in before.items()}, "the state is not modified")
        note("replay kernels", f"{case['name']} S={S} {'chunked' if case['M'] > 112 else 'one chunk'}")


# ---------------------------------------------------------------------------------------------------------------------
# (c) per-step decode kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_decode_step_kernel_follows_the_rule(name):
    """decode_step(mode="evaluate", fuse_env_step=True) on the zero cache: finite logits == the mask before the step, the
    state after it == step_ref's.  Slot-major at the named size, plane-major at M = 129."""
    from eam_rl4co_amd import ops

    env_name = step_cases.case_by_name(name)["env"]
    for M, S, planes in [(None, 1, False), (None, 4, False), (129, 4, True)]:
        ref = reference(name, M, S)
        case, hist, actions = ref["case"], ref["hist"], ref["actions"]
        st = upload(case, hist[0])
        cache = zero_cache(case, planes)
        acts = t(actions.T.copy())
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        snaps, finite, lps = [device_slots(st)], [], []
        for k in range(actions.shape[1]):
            _, lp, _, logits, _ = ops.decode_step(st, cache, mode="evaluate", given=acts[k], fuse_env_step=True,
                                                  want_logits=True, status=status)
            finite.append(torch.isfinite(logits))
            lps.append(lp)
            snaps.append(device_slots(st))
        want = stacked_expected(case, hist)
        live = ~want["done"][:-1]          # a finished PDP / TSP row has no feasible node: its logits are not defined
        got_finite = torch.stack(finite).cpu().numpy()
        assert_bits_equal(got_finite[live], want["mask"][:-1][live], f"{case['name']}: isfinite(logits) vs mask")
        if env_name not in ("tsp", "pdp"):
            assert_bits_equal(got_finite, want["mask"][:-1], f"{case['name']}: isfinite(logits) vs mask (finished rows too)")
        assert_state_equal(stacked(snaps), want, f"{case['name']} S={S} planes={planes}")
        count = np.exp(-torch.stack(lps).cpu().numpy().astype(np.float64))
        assert (np.abs(count - ref["counts"].T)[live] < 0.25).all(), "exp(-logp) vs the feasible count"
        assert int(status.item()) == 0
        note("decode step", f"{case['name']} S={S} {'plane-major' if planes else 'slot-major'}")


# ---------------------------------------------------------------------------------------------------------------------
# (d), (e), (f) whole-rollout kernels
# ---------------------------------------------------------------------------------------------------------------------
KERNELS = ("ms_mfma", "resident", "stream")


class forced:
    """Force one rollout kernel with the library's switches: 11 turns the start-sharing MFMA kernel off, 1 the resident one."""

    def __init__(self, kernel):
        self.keys = {"ms_mfma": (), "resident": (11,), "stream": (11, 1)}[kernel]

    def __enter__(self):
        from eam_rl4co_amd import _lib

        for k in self.keys:
            assert _lib.load().eamrl_debug_set(k, 1) == 0

    def __exit__(self, *exc):
        from eam_rl4co_amd import _lib

        for k in self.keys:
            _lib.load().eamrl_debug_set(k, 0)


def supported(kernel, env, M, S):
    """What rollout_ms_mfma_supports / rollout_resident_supports admit at E = 128, H = 8 without a filter."""
    if kernel == "ms_mfma":
        return S >= 2 and M <= 112 and env != "pdp"
    if kernel == "resident":
        return M <= 128
    return True


def run_rollout(case, states, prefs, kernel, mode="sampling", given=None):
    """One ops.rollout on the zero cache under a forced kernel -> (actions, logps, steps, status, final device slots)."""
    from eam_rl4co_amd import ops

    st = upload(case, states)
    cache = zero_cache(case, planes=case["M"] > 128)
    T = prefs.shape[1]
    with forced(kernel):
        assert ops.rollout_kernel(st, cache, st.R, T) == kernel, f"{case['name']}: {kernel} is not the kernel that runs"
        kw = dict(noise=t(step_cases.noise_from_prefs(prefs))) if mode == "sampling" else dict(given=t(given))
        actions, logps, info = ops.rollout(st, cache, mode=mode, t_max=T, **kw)
        info = info.cpu().numpy()
    return actions.cpu().numpy(), logps.cpu().numpy(), int(info[0]), int(info[1]), device_slots(st)


def check_rollout(case, ref_actions, ref_counts, final_states, out, what):
    actions, logps, steps, status, final = out
    T = ref_actions.shape[1]
    assert status == 0, f"{what}: status {status}"
    assert steps == T, f"{what}: {steps} steps, the reference takes {T}"
    assert_bits_equal(actions[:, :T], ref_actions, f"{what}: actions")
    assert not actions[:, T:].any()
    count = np.exp(-logps[:, :T].astype(np.float64))
    worst = np.abs(count - ref_counts).max()
    assert worst < 0.25, f"{what}: exp(-logp) is {worst} away from the feasible count"
    assert_state_equal(final, expected_slots(case, final_states), f"{what}: final state")


def combos(name):
    """(M, S, kernel) to run for a case, in a fixed order."""
    env = step_cases.case_by_name(name)["env"]
    out = []
    for M, S in sizes_for(name):
        size = M or step_cases.case_by_name(name)["M"]
        out += [(M, S, k) for k in KERNELS if supported(k, env, size, S)]
    return out


def test_rollout_combinations_are_the_expected_ones():
    """No kernel silently drops out: the combinations the rollout tests run, against an explicit list."""
    depot = [(None, 1, "resident"), (None, 1, "stream"), (None, 4, "ms_mfma"), (None, 4, "resident"), (None, 4, "stream"),
             (65, 4, "ms_mfma"), (65, 4, "resident"), (65, 4, "stream"), (112, 4, "ms_mfma"), (112, 4, "resident"),
             (112, 4, "stream"), (113, 4, "resident"), (113, 4, "stream"), (128, 4, "resident"), (128, 4, "stream"),
             (129, 4, "stream")]
    pdp = [(None, 1, "resident"), (None, 1, "stream"), (None, 4, "resident"), (None, 4, "stream"), (65, 4, "resident"),
           (65, 4, "stream"), (113, 4, "resident"), (113, 4, "stream"), (129, 4, "stream")]
    for name in NAMES:
        assert combos(name) == (pdp if name.startswith("pdp") else depot), name


@pytest.mark.parametrize("name", NAMES)
def test_rollout_kernels_follow_the_rule(name):
    """(d) sampling with the rank noise on each forced kernel: actions, feasible counts, step count, status and the written-back
    final state of every row, rows that finished early included."""
    ran = []
    for M, S, kernel in combos(name):
        ref = reference(name, M, S)
        out = run_rollout(ref["case"], ref["hist"][0], ref["prefs"], kernel)
        check_rollout(ref["case"], ref["actions"], ref["counts"], ref["hist"][-1], out, f"{ref['case']['name']} S={S} {kernel}")
        ran.append((M, S, kernel))
    assert ran == combos(name)
    note("rollout kernels", f"{name}: {ran}")


def mid_steps(ref):
    """k = 1, the first k >= 2 that leaves row 0 at a customer, the first k just after row 0 returned to the depot."""
    a = ref["actions"][0]
    ks = [1]
    ks += [k for k in range(2, len(a)) if a[k - 1] != 0][:1]
    ks += [k for k in range(2, len(a)) if a[k - 1] == 0][:1]
    return sorted(set(ks))


@pytest.mark.parametrize("name", NAMES)
def test_rollout_kernels_start_from_a_mid_episode_state(name):
    """(f) the state after k scripted steps uploaded, the rollout continued from there: what the kernels derive from the
    incoming planes (visit counts, step counters, the clock) must continue the episode as step_ref does."""
    env = step_cases.case_by_name(name)["env"]
    for M, S in [(None, 4), (65, 4), (129, 4)]:
        ref = reference(name, M, S)
        case = ref["case"]
        for k in mid_steps(ref):
            if k >= ref["actions"].shape[1]:
                continue
            prefs = ref["prefs"][:, k:]
            acts, counts, final, _ = step_ref.rollout_first_feasible(case["batch"], prefs, start_state=ref["hist"][k])
            assert np.array_equal(acts, ref["actions"][:, k:])
            for kernel in KERNELS:
                if supported(kernel, env, case["M"], S):
                    out = run_rollout(case, ref["hist"][k], prefs, kernel)
                    check_rollout(case, acts, counts, final, out, f"{case['name']} from step {k} on {kernel}")
                    note("mid-episode start", f"{case['name']} k={k} {kernel}")


@pytest.mark.parametrize("name", NAMES)
def test_teacher_forced_rollouts_follow_the_rule(name):
    """(e) mode="evaluate" on the reference trajectory: same counts, status 0; with the node the reference judges infeasible by
    one float32 step forced at the boundary step: ST_INFEASIBLE (the at-boundary node is part of the reference trajectory)."""
    from eam_rl4co_amd import ops

    env = step_cases.case_by_name(name)["env"]
    pair = step_cases.BOUNDARY_PAIRS.get(name)
    for M, S in [(None, 4), (129, 4)]:
        ref = reference(name, M, S)
        case, actions = ref["case"], ref["actions"]
        nm = step_cases.node_map(step_cases.case_by_name(name)["M"], case["M"]) if M else None
        for kernel in KERNELS:
            if not supported(kernel, env, case["M"], S):
                continue
            out = run_rollout(case, ref["hist"][0], ref["prefs"][:, :actions.shape[1]], kernel, "evaluate", actions)
            check_rollout(case, actions, ref["counts"], ref["hist"][-1], out, f"{case['name']} teacher-forced on {kernel}")
            if pair:
                (b_ok, k_ok, n_ok), (b_bad, k_bad, n_bad) = pair
                n_ok, n_bad = (int(nm[n_ok]), int(nm[n_bad])) if M else (n_ok, n_bad)
                assert actions[b_ok, k_ok] == n_ok and ref["hist"][k_ok][b_ok]["mask"][n_ok]
                assert not ref["hist"][k_bad][b_bad]["mask"][n_bad]
                bad = actions.copy()
                bad[b_bad::3, k_bad] = n_bad
                status = run_rollout(case, ref["hist"][0], ref["prefs"][:, :actions.shape[1]], kernel, "evaluate", bad)[3]
                assert status & ops.ST_INFEASIBLE, f"{case['name']} on {kernel}: the infeasible node went unnoticed"
            note("teacher forcing", f"{case['name']} {kernel}{' + infeasible probe' if pair else ''}")


def test_report_what_was_exercised():
    """Lists, per test, the cases, sizes and kernels that ran (shown with -s / -rA)."""
    for test, items in EXERCISED.items():
        print(f"{test}: {len(items)} runs")
        for it in items:
            print("   ", it)
