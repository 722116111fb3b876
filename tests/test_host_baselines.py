"""CPU: the REINFORCE baselines (eam_rl4co_amd/baselines.py), the loss steps built on them and the epoch logic, against
fixtures recorded from the reference (tests/golden/make_golden_baselines.py) and with stub policies where a rollout is needed."""
import json
import os
import pickle
import socket

import numpy as np
import pytest
import torch
import torch.nn as nn

from _util import GOLDEN, golden

import eam_rl4co_amd as ea
from eam_rl4co_amd import baselines as bl
from eam_rl4co_amd import train


@pytest.fixture(scope="module")
def fx():
    return golden("baselines_host")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


# float32 results recorded from the same torch expressions on the same CPU: a last-bit tolerance (4 ulp of the value)
def close32(got, want):
    want = np.asarray(want)
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), want.astype(np.float64), rtol=4 * 2.0 ** -23, atol=1e-30)


# ------------------------------------------------------------------------------------------------------------
# value sequences
# ------------------------------------------------------------------------------------------------------------
def test_exponential_and_mean_sequences(fx):
    for tag, b in (("exp08", ea.ExponentialBaseline(0.8)), ("mean", ea.MeanBaseline())):
        assert isinstance(b, ea.ExponentialBaseline)
        for r, want in zip(fx["seq_rewards"], fx[f"seq_{tag}"]):
            v, loss = b.eval(None, T(r))
            assert loss == 0 and v.dim() == 0
            close32(v, want)
    assert ea.ExponentialBaseline().beta == 0.8 and ea.MeanBaseline().beta == 0.0
    assert ea.NoBaseline().eval(None, T(fx["seq_rewards"][0])) == (0, 0)
    v, loss = ea.SharedBaseline().eval(None, torch.arange(6.0).view(2, 3))
    assert loss == 0 and v.shape == (2, 1) and v.flatten().tolist() == [1.0, 4.0]


class ConstBaseline(bl.REINFORCEBaseline):
    """(the stub of the fixture: per-row value 2 * row index, loss 0.25; counts its callbacks)"""

    calls = 0
    wrapped = 0

    def eval(self, td, reward, env=None):
        return torch.arange(reward.shape[0], dtype=reward.dtype) * 2.0, torch.tensor(0.25)

    def epoch_callback(self, *a, **kw):
        self.calls += 1

    def wrap_dataset(self, dataset, *a, **kw):
        self.wrapped += 1
        return dataset


def test_warmup_schedule_values_and_delegation(fx):
    inner = ConstBaseline()
    wb = ea.WarmupBaseline(inner, n_epochs=2, warmup_exp_beta=0.8)
    assert wb.alpha == 0 and isinstance(wb.warmup_baseline, ea.ExponentialBaseline) and wb.warmup_baseline.beta == 0.8
    i = 0
    for epoch in range(3):
        wb.wrap_dataset("ds")
        assert inner.wrapped == epoch               # delegates only once alpha > 0 (epochs 1, 2)
        for r in fx["seq_rewards"][:2]:
            v, loss = wb.eval(None, T(r))
            close32(torch.as_tensor(v, dtype=torch.float32).expand(6), fx["warmup_vals"][i])
            close32(float(loss), fx["warmup_losses"][i])
            i += 1
        wb.epoch_callback(epoch=epoch)
        assert inner.calls == epoch + 1             # the inner callback runs every epoch
        assert wb.alpha == fx["warmup_alphas"][epoch] == min((epoch + 1) / 2, 1.0)
    with pytest.raises(AssertionError):
        ea.WarmupBaseline(inner, n_epochs=0)


# ------------------------------------------------------------------------------------------------------------
# calculate_loss shapes
# ------------------------------------------------------------------------------------------------------------
class FixedPolicy:
    """policy(td, env, ...) -> fixed rows"""

    def __init__(self, reward, logp):
        self.reward, self.logp = reward, logp

    def __call__(self, td, env, **kw):
        return {"actions": torch.zeros(self.reward.shape[0], self.logp.shape[1], dtype=torch.int64), "reward": self.reward,
                "log_likelihood": self.logp}


def _loss(fx, tag, baseline, num_starts=0, reward_scale=None):
    r, ll = T(fx[f"{tag}__reward"]), T(fx[f"{tag}__ll"])
    extra = T(fx[f"{tag}__extra"]) if f"{tag}__extra" in fx else None
    if num_starts > 1:        # rows in (s b) order; the per-step log-probs are one column
        pol = FixedPolicy(r.t().reshape(-1), ll.t().reshape(-1, 1).clone().requires_grad_())
    else:
        pol = FixedPolicy(r.reshape(-1), ll.reshape(-1, 1).clone().requires_grad_())
    out = train.reinforce_loss(pol, None, {}, baseline=baseline, num_starts=num_starts, extra=extra, reward_scale=reward_scale)
    return out, pol


def test_reinforce_loss_bl_val_shape_cases(fx):
    for tag, baseline, kw in (("rf_scalar", ea.get_reinforce_baseline("rollout"), {}), ("rf_extra_b", "no", {}),
                              ("rf_extra_b", ea.NoBaseline(), {}), ("rf_shared", ea.SharedBaseline(), dict(num_starts=3)),
                              ("rf_norm", None, dict(reward_scale="norm"))):
        out, pol = _loss(fx, tag, baseline, **kw)
        if tag == "rf_norm":        # the recorded advantage carries the rounding of float32 running sums (see close_scaled): 4 values,
            # |x| <= 8: each standardised advantage is good to about 2e-6, times |ll| <= 30 and averaged: 6e-5 on a loss of 2
            np.testing.assert_allclose(float(out["loss"].detach()), float(fx[f"{tag}__loss"]), rtol=0, atol=6e-5)
            continue
        close32(out["loss"].detach(), fx[f"{tag}__loss"])
        close32(out["reinforce_loss"].detach(), fx[f"{tag}__reinforce_loss"])
        close32(torch.as_tensor(out["bl_val"]), fx[f"{tag}__bl_val"])
        assert torch.as_tensor(out["bl_val"]).shape == fx[f"{tag}__bl_val"].shape
        assert float(torch.as_tensor(out["bl_loss"])) == float(fx[f"{tag}__bl_loss"])
        out["loss"].backward()
        assert pol.logp.grad is not None and torch.isfinite(pol.logp.grad).all()
    # [B, 1] extra against [B] rewards would broadcast to [B, B]: the fixture's [B, 1] case has [B, 1] rewards and equals the [B] one
    assert float(fx["rf_extra_b1__loss"]) == float(fx["rf_extra_b__loss"])
    r, ll, ex = T(fx["rf_extra_b1__reward"]), T(fx["rf_extra_b1__ll"]), T(fx["rf_extra_b1__extra"])
    out = train._calculate_loss(ea.NoBaseline(), None, None, None, {}, r, ll, ex)
    close32(out["loss"], fx["rf_extra_b1__loss"])
    assert out["bl_val"].shape == (4, 1)


def test_eam_calculate_loss_shape_cases(fx):
    """EAM.calculate_loss: a 1-D value of half the rows is concatenated with itself -- against [2B, 1] rewards the advantage is
    then [2B, 2B] (every row minus every instance's value); B = 4, so any other broadcast changes the number."""
    assert int(fx["has_eam"]) == 1
    for tag, baseline in (("eam_extra_b", ea.NoBaseline()), ("eam_extra_2b", ea.NoBaseline()),
                          ("eam_scalar_2b", ea.get_reinforce_baseline("rollout"))):
        r, ll = T(fx[f"{tag}__reward"]), T(fx[f"{tag}__ll"])
        extra = T(fx[f"{tag}__extra"]) if f"{tag}__extra" in fx else None
        out = train._calculate_loss(baseline, None, None, None, {}, r, ll, extra, eam_shapes=True)
        close32(out["loss"], fx[f"{tag}__loss"])
        assert torch.as_tensor(out["bl_val"]).shape == fx[f"{tag}__bl_val"].shape
        close32(torch.as_tensor(out["bl_val"]), fx[f"{tag}__bl_val"])
    r, ll, ex = T(fx["eam_extra_2b__reward"]), T(fx["eam_extra_2b__ll"]), T(fx["eam_extra_2b__extra"])
    rowwise = -((r - torch.cat([ex, ex])[:, None]) * ll).mean()
    assert abs(float(rowwise) - float(fx["eam_extra_2b__loss"])) > 1e-2          # the row-wise broadcast is NOT what is computed
    eff = -((r - ex.mean()) * ll).mean()                                          # ... the batch mean of the values is
    np.testing.assert_allclose(float(eff), float(fx["eam_extra_2b__loss"]), rtol=1e-5)


class EamStubPolicy(nn.Module):
    """Sampled call -> fixed rows; actions= -> rewards + 1, log-likelihood * 0.5."""

    def __init__(self, reward, ll):
        super().__init__()
        self.w = nn.Parameter(torch.ones(()))
        self.reward, self.ll = reward, ll
        self._shared_dt = None

    def forward(self, td, env, actions=None, **kw):
        if actions is None:
            return {"actions": torch.arange(4).repeat(self.reward.shape[0], 1), "reward": self.reward, "log_likelihood": self.ll * self.w,
                    "entropy": torch.zeros_like(self.reward)}
        return {"actions": actions, "reward": self.reward + 1.0, "log_likelihood": self.ll * 0.5 * self.w}


def test_eam_am_loss_on_stubs(fx, monkeypatch):
    from eam_rl4co_amd import evolution

    B = 4
    r, ll = T(fx["rf_extra_b__reward"]), T(fx["rf_extra_b__ll"])
    ex = T(fx["rf_extra_b__extra"])
    monkeypatch.setattr(evolution, "evolution_worker", lambda actions, td, runner, env, draws=None, generator=None: (actions.flip(1), None))
    pol = EamStubPolicy(r, ll)
    td = ea.TensorDict({"locs": torch.rand(B, 4, 2)}, batch_size=[B])
    out = ea.eam_am_loss(pol, None, td, None, ea.NoBaseline(), extra=ex)
    r2, l2 = torch.cat([r, r + 1.0])[:, None], torch.cat([ll, ll * 0.5])[:, None]
    want = -((r2 - torch.cat([ex, ex])) * l2).mean()
    assert out["bl_val"].shape == (2 * B,) and torch.equal(out["loss"].detach(), want)
    assert torch.equal(out["improved_actions"], out["actions"].flip(1)) and torch.equal(out["improved_reward"], r + 1.0)
    out["loss"].backward()
    assert pol.w.grad is not None and float(pol.w.grad) != 0.0
    # without improvement: the loss of the sampled rows alone, extra unsqueezed to [B, 1]
    out = ea.eam_am_loss(pol, None, td, None, ea.NoBaseline(), extra=ex, improve=False)
    assert out["bl_val"].shape == (B, 1) and torch.equal(out["loss"].detach(), -((r - ex) * ll).mean())
    # evaluated on the fly, the baseline is asked twice per step, as the reference's two calculate_loss calls do
    e = ea.ExponentialBaseline(0.8)
    out = ea.eam_am_loss(pol, None, td, None, e)
    v1 = r.mean()
    v2 = 0.8 * v1 + (1.0 - 0.8) * r2.mean()
    assert torch.equal(e.v, v2) and torch.equal(out["loss"].detach(), -((r2 - v2) * l2).mean())


def close_scaled(got, want, x, n_seen):
    """The recording is the reference's float32 arithmetic on running sums over the n_seen values so far: its mean is good to
    n_seen half-ulps of the largest |x|, its standard deviation to n_seen ulps relative.  The statistics here are float64, so the
    difference is the recording's own rounding: |d mean| / std + |want| * (d std / std), plus one ulp for the final division."""
    x = np.asarray(x, dtype=np.float64)
    xmax, std = np.abs(x).max(), x.std(ddof=1)
    atol = n_seen * 2.0 ** -24 * xmax / std
    rtol = (n_seen + 1) * 2.0 ** -23
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), rtol=rtol, atol=atol)


def test_reward_scaler_sequences(fx):
    for scale in ("norm", "scale", 3):
        sc = ea.RewardScaler(scale)
        for i, (x, want) in enumerate(zip(fx["scaler_in"], fx[f"scaler_{scale}"])):
            x = T(x).clone()
            keep = x.clone()
            got = sc(x)
            assert got.dtype == torch.float32
            if scale == 3:
                close32(got, want)
            else:
                close_scaled(got, want, fx["scaler_in"][:i + 1], 5 * (i + 1))
            assert torch.equal(x, keep)            # the input is left alone
        if scale != 3:     # the statistics are those of everything seen
            allx = fx["scaler_in"].astype(np.float64).reshape(-1)
            assert sc.count == allx.size
            np.testing.assert_allclose(float(sc.mean), allx.mean(), rtol=1e-12)
            np.testing.assert_allclose(float(sc.M2), ((allx - allx.mean()) ** 2).sum(), rtol=1e-12)
    x0 = T(fx["scaler_in"][0])
    assert ea.RewardScaler(None)(x0) is x0
    with pytest.raises(ValueError):
        ea.RewardScaler("nonsense")(torch.ones(3))


# ------------------------------------------------------------------------------------------------------------
# paired t-test
# ------------------------------------------------------------------------------------------------------------
# float64 throughout; the statistic is a mean over a standard deviation of n <= 64 numbers (a few ulp), the p-value a
# continued fraction converged to 1e-16 times exp(lgamma terms of size <= 1e3, each good to ~1e-15 relative): 1e-12 / 1e-9
def test_paired_ttest_against_recorded_scipy(fx):
    for k in fx["tt_names"]:
        a, b, (t_ref, p_ref) = fx[f"tt_{k}__a"], fx[f"tt_{k}__b"], fx[f"tt_{k}__tp"]
        t, p = ea.paired_ttest(a, b)
        assert isinstance(t, float) and isinstance(p, float)
        if np.isinf(t_ref):
            assert t == t_ref and p == 0.0
            continue
        np.testing.assert_allclose(t, t_ref, rtol=1e-7 if k == "tiny_var" else 1e-12)   # tiny_var: SciPy itself warns of cancellation
        np.testing.assert_allclose(p, p_ref, rtol=1e-9, atol=1e-300)
        t2, p2 = ea.paired_ttest(torch.from_numpy(b), torch.from_numpy(a))
        assert t2 == -t and p2 == p
    assert all(np.isnan(v) for v in ea.paired_ttest([1.0], [2.0]))
    assert all(np.isnan(v) for v in ea.paired_ttest([1.0, 2.0], [1.0, 2.0]))
    with pytest.raises(ValueError):
        ea.paired_ttest([1.0, 2.0], [1.0])


def test_paired_ttest_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(0)
    for n in (2, 3, 10, 101, 1000, 10000):
        for shift in (0.0, 0.01, 0.3):
            a = rng.normal(-8, 1, n)
            b = a + rng.normal(shift, 0.2, n)
            t_ref, p_ref = stats.ttest_rel(a, b)
            t, p = ea.paired_ttest(a, b)
            np.testing.assert_allclose(t, t_ref, rtol=1e-12)
            np.testing.assert_allclose(p, p_ref, rtol=1e-9, atol=1e-300)


def test_no_scipy_import_at_run_time():
    import subprocess
    import sys

    code = ("import sys; import eam_rl4co_amd as ea; ea.paired_ttest([1.0, 2.0, 4.0], [1.5, 2.0, 3.0]); "
            "assert not any(m == 'scipy' or m.startswith('scipy.') for m in sys.modules), 'scipy imported'")
    root = os.path.dirname(os.path.dirname(GOLDEN))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]


# ------------------------------------------------------------------------------------------------------------
# registry
# ------------------------------------------------------------------------------------------------------------
def _describe(b):
    d = {"class": type(b).__name__}
    for k in ("beta", "alpha", "n_epochs", "bl_alpha"):
        if hasattr(b, k):
            d[k] = getattr(b, k)
    for k in ("baseline", "warmup_baseline"):
        if isinstance(getattr(b, k, None), bl.REINFORCEBaseline):
            d[k] = _describe(getattr(b, k))
    if hasattr(b, "critic"):
        d["critic"] = None if b.critic is None else type(b.critic).__name__
    return d


def test_get_reinforce_baseline_structures():
    with open(os.path.join(GOLDEN, "baselines_structs.json")) as f:
        ref = json.load(f)
    assert sorted(ea.REINFORCE_BASELINES_REGISTRY) == ref.pop("registry") and "rollout_only" in ea.REINFORCE_BASELINES_REGISTRY
    assert ref.pop("unknown_raises") == "ValueError"
    with pytest.raises(ValueError):
        ea.get_reinforce_baseline("nonsense")
    for case in ref.values():
        assert _describe(ea.get_reinforce_baseline(case["name"], **case["kwargs"])) == case["structure"], case
    # "warmup" with an inner name or object (the reference's call raises TypeError there: its keyword arrives twice)
    w = ea.get_reinforce_baseline("warmup", baseline="exponential", n_epochs=2)
    assert isinstance(w, ea.WarmupBaseline) and isinstance(w.baseline, ea.ExponentialBaseline) and w.n_epochs == 2
    inner = ea.RolloutBaseline(bl_alpha=0.2)
    assert ea.get_reinforce_baseline("warmup", baseline=inner).baseline is inner


# ------------------------------------------------------------------------------------------------------------
# RolloutBaseline with stub policies
# ------------------------------------------------------------------------------------------------------------
class StubEnv:
    """dataset -> locs + idx (the position of an instance in its dataset); reset -> the rows as they are."""

    name = "stub"

    def __init__(self):
        self.made = 0

    def dataset(self, batch_size=[]):
        n = batch_size[0]
        self.made += 1
        g = torch.Generator().manual_seed(100 + self.made)
        return ea.TensorDictDataset(ea.TensorDict({"locs": torch.rand(n, 5, 2, generator=g), "idx": torch.arange(n)}, batch_size=[n]))

    def reset(self, td):
        return td


class StubPolicy(nn.Module):
    """reward = -sum(locs) + offsets[idx]; records the modes and chunk sizes it was called with."""

    def __init__(self, offsets):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(()))
        self.offsets = offsets
        self.log = []

    def forward(self, td, env, decode_type=None, **kw):
        assert decode_type == "greedy" and not torch.is_grad_enabled() and not torch.is_inference_mode_enabled()
        self.log.append((self.training, td.batch_size[0]))
        return {"reward": (-td["locs"].sum((1, 2)) + self.offsets[td["idx"]] + self.w).float()}


N = 64
ALT = torch.tensor([1.0, -1.0]).repeat(N // 2)


def _setup(bl_alpha=0.05):
    env = StubEnv()
    base = StubPolicy(torch.zeros(N))
    rb = ea.RolloutBaseline(bl_alpha=bl_alpha)
    rb.setup(base, env, batch_size=7, device="cpu", dataset_size=N)
    return env, base, rb


def test_rollout_baseline_setup_and_rollout():
    env, base, rb = _setup()
    assert rb.policy is not base and not rb.policy.training and not any(p.requires_grad for p in rb.policy.parameters())
    assert base.training and base.w.requires_grad
    assert hasattr(rb.dataset, "batch_size") and rb.dataset.batch_size[0] == N            # ONE TensorDict, not a list of dicts
    assert rb.bl_vals.dtype == np.float64 and rb.bl_vals.shape == (N,) and rb.mean == float(rb.bl_vals.mean())
    assert [c for _, c in rb.policy.log] == [7] * 9 + [1]
    base.train()
    r = rb.rollout(base, env, batch_size=64, device="cpu")
    assert r.dtype == torch.float32 and r.shape == (N,) and base.training and base.log[-1] == (False, 64)      # mode restored
    base.eval()
    rb.rollout(base, env, 64, "cpu")
    assert not base.training
    assert torch.equal(r, rb.rollout(base, env, 7, "cpu")) and np.array_equal(r.numpy().astype(np.float64), rb.bl_vals)
    v, loss = rb.eval(env.reset(rb.dataset[:5]), None, env)
    assert loss == 0 and torch.equal(v, r[:5])


def test_rollout_baseline_epoch_decisions(monkeypatch):
    # significantly better -> updated, with a new evaluation dataset and the candidate's weights
    env, base, rb = _setup()
    cand = StubPolicy(0.5 + 0.01 * ALT)
    old_ds = rb.dataset
    assert rb.epoch_callback(cand, env=env, batch_size=16, device="cpu", epoch=0, dataset_size=N) is True
    assert rb.dataset is not old_ds and not torch.equal(rb.dataset["locs"], old_ds["locs"]) and env.made == 2
    assert torch.equal(rb.policy.offsets, cand.offsets) and rb.policy is not cand and not rb.policy.training
    assert np.array_equal(rb.bl_vals, rb.rollout(cand, env, 64, "cpu").numpy().astype(np.float64))
    # better, but not significantly (mean +0.01 with unit spread: one-sided p = 0.47) -> kept
    env, base, rb = _setup()
    cand = StubPolicy(0.01 + ALT)
    pol, ds, vals = rb.policy, rb.dataset, rb.bl_vals.copy()
    t, p = ea.paired_ttest(-(vals + cand.offsets.numpy()), -vals)
    assert t < 0 and 0.05 < p / 2 < 0.5
    assert rb.epoch_callback(cand, env=env, batch_size=16, device="cpu", epoch=0, dataset_size=N) is False
    assert rb.policy is pol and rb.dataset is ds and np.array_equal(rb.bl_vals, vals) and env.made == 1
    # ... and updated under a bl_alpha above that p
    env, base, rb = _setup(bl_alpha=0.6)
    assert rb.epoch_callback(cand, env=env, batch_size=16, device="cpu", epoch=0, dataset_size=N) is True
    # worse (or equal) -> the test is not run
    env, base, rb = _setup()
    monkeypatch.setattr(bl, "paired_ttest", lambda *a: (_ for _ in ()).throw(AssertionError("t-test run")))
    assert rb.epoch_callback(StubPolicy(torch.full((N,), -0.5)), env=env, batch_size=16, device="cpu", epoch=0, dataset_size=N) is False
    assert rb.epoch_callback(StubPolicy(torch.zeros(N)), env=env, batch_size=16, device="cpu", epoch=0, dataset_size=N) is False
    assert env.made == 1


def test_rollout_baseline_needs_an_evaluation_dataset_of_two():
    env, base = StubEnv(), StubPolicy(torch.zeros(N))
    for size in (None, 0, 1):
        with pytest.raises(ValueError, match="at least 2"):
            ea.RolloutBaseline().setup(base, env, batch_size=7, device="cpu", dataset_size=size)
    step = ea.PolicyGradientStep(ea.AttentionModelPolicy(env_name="tsp", num_encoder_layers=1), env, baseline="rollout")
    with pytest.raises(ValueError, match="val_data_size"):
        step.setup(batch_size=8)


def test_dataset_builds_its_item_list_on_demand():
    ds = StubEnv().dataset([6])
    assert ds._data is None and len(ds) == 6
    from eam_rl4co_amd.baselines import as_tensordict

    assert as_tensordict(ds) is ds.td and ds._data is None          # whole-dataset consumers never build the list
    wrapped = ds.add_key("extra", torch.arange(6.0))
    assert ds._data is None and wrapped.td["extra"].tolist() == list(range(6))
    assert torch.equal(ds[2]["locs"], ds.td["locs"][2]) and len(ds.data) == 6 and wrapped.data is ds.data


def test_rollout_baseline_pickles_without_its_dataset():
    env, base, rb = _setup()
    back = pickle.loads(pickle.dumps(rb))
    assert back.dataset is None and np.array_equal(back.bl_vals, rb.bl_vals) and back.mean == rb.mean and back.bl_alpha == rb.bl_alpha
    assert torch.equal(back.policy.offsets, rb.policy.offsets) and not back.policy.training
    with pytest.raises(RuntimeError, match="setup"):
        back.rollout(base, env, 8, "cpu")
    back.setup(base, env, batch_size=8, device="cpu", dataset_size=N)
    assert back.dataset is not None
    w = pickle.loads(pickle.dumps(ea.WarmupBaseline(rb, n_epochs=2)))
    assert w.baseline.dataset is None and w.alpha == 0


def test_add_key_collate_and_wrap_dataset():
    env, base, rb = _setup()
    ds = env.dataset([10])
    values = torch.arange(10.0)
    wrapped = ds.add_key("extra", values)
    assert isinstance(wrapped, ea.ExtraKeyDataset) and len(wrapped) == 10
    batch = wrapped.collate_fn([wrapped[i] for i in (3, 4, 7)])
    assert batch["extra"].tolist() == [3.0, 4.0, 7.0] and batch.batch_size[0] == 3 and torch.equal(batch["locs"], ds.td["locs"][[3, 4, 7]])
    loader = torch.utils.data.DataLoader(wrapped, batch_size=4, collate_fn=wrapped.collate_fn)
    assert [b["extra"].tolist() for b in loader] == [[0.0, 1.0, 2.0, 3.0], [4.0, 5.0, 6.0, 7.0], [8.0, 9.0]]
    with pytest.raises(AssertionError):
        ds.add_key("extra", torch.zeros(9))
    # wrap_dataset: a dataset stays a dataset, a TensorDict a TensorDict; both carry the frozen copy's greedy rewards
    ds = env.dataset([12])
    want = rb.rollout(rb.policy, env, 5, "cpu", dataset=ds)
    w1 = rb.wrap_dataset(ds, env, batch_size=5, device="cpu")
    assert isinstance(w1, ea.ExtraKeyDataset) and torch.equal(w1.extra, want) and torch.equal(w1[2]["extra"], want[2])
    w2 = rb.wrap_dataset(ds.td, env, batch_size=5, device="cpu")
    assert hasattr(w2, "batch_size") and torch.equal(w2["extra"], want) and "extra" not in ds.td.keys()
    # the warm-up hands the dataset through untouched while alpha == 0
    warm = ea.WarmupBaseline(rb)
    assert warm.wrap_dataset(ds, env, batch_size=5, device="cpu") is ds
    warm.alpha = 1.0
    assert torch.equal(warm.wrap_dataset(ds, env, batch_size=5, device="cpu").extra, want)


# ------------------------------------------------------------------------------------------------------------
# two ranks: rank 0's verdict holds
# ------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _verdict_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    from eam_rl4co_amd import dist as ed

    ed.init_distributed("gloo")
    results = []
    # case 0: rank 0 sees a significantly better candidate, rank 1 a worse one; case 1: the other way round
    for case in range(2):
        env, base, rb = _setup()
        better = (rank == 0) == (case == 0)
        cand = StubPolicy(0.5 + 0.01 * ALT if better else torch.full((N,), -0.5))
        updated = rb.epoch_callback(cand, env=env, batch_size=16, device="cpu", epoch=0, dataset_size=N)
        results.append((better, bool(updated), bool(torch.equal(rb.policy.offsets, cand.offsets)), env.made))
    dist.barrier()
    dist.destroy_process_group()
    out.put((rank, results))


def test_two_ranks_follow_rank0_verdict():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_verdict_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0, f"rank exited with {p.exitcode}"
    res = dict(out.get(timeout=5) for _ in range(2))
    # case 0: rank 0 alone updates, rank 1 alone would not -> both updated; case 1: the reverse -> neither
    assert res[0][0] == (True, True, True, 2) and res[1][0] == (False, True, True, 2)
    assert res[0][1] == (False, False, False, 1) and res[1][1] == (True, False, False, 1)


# ------------------------------------------------------------------------------------------------------------
# the step object and the loop, and the four old strings
# ------------------------------------------------------------------------------------------------------------
def test_policy_gradient_step_hooks_are_noops_for_the_old_strings():
    pol = ea.AttentionModelPolicy(env_name="tsp", num_encoder_layers=1)
    step = ea.PolicyGradientStep(pol, env=None, num_starts=0)
    assert step.baseline == "mean"
    ds = object()
    step.setup(batch_size=8, dataset_size=16)
    assert step.wrap_dataset(ds) is ds
    step.on_epoch_end(0)
    assert ea.PolicyGradientStep(pol, env=None, num_starts=4).baseline == "shared"
    s2 = ea.PolicyGradientStep(pol, env=None, baseline="rollout", baseline_kwargs=dict(n_epochs=2, bl_alpha=0.1))
    assert isinstance(s2.baseline, ea.WarmupBaseline) and s2.baseline.n_epochs == 2 and s2.baseline.baseline.bl_alpha == 0.1
    inner = ea.ExponentialBaseline(0.5)
    assert ea.PolicyGradientStep(pol, env=None, baseline=inner).baseline is inner
    with pytest.raises(ValueError):
        ea.PolicyGradientStep(pol, env=None, baseline="nonsense")
    with pytest.raises(NotImplementedError):
        ea.PolicyGradientStep(pol, env=None, baseline=ea.CriticBaseline())


def test_the_four_old_baseline_strings_are_unchanged():
    reward = torch.tensor([-3.0, -5.0, -4.0, -6.5, -2.0, -7.0])
    logp = torch.tensor([[-1.0, -2.0], [-0.5, -0.25], [-3.0, 0.0], [-1.5, -1.0], [-0.125, -2.5], [-4.0, -0.5]])
    ll = logp.sum(1)
    pol = FixedPolicy(reward, logp)
    keys = {"loss", "reward", "log_likelihood", "actions", "logp_steps", "native_log_likelihood"}
    out = train.reinforce_loss(pol, None, {}, baseline="mean")
    assert set(out) == keys and torch.equal(out["loss"], -((reward - reward.mean()) * ll).mean())
    out = train.reinforce_loss(pol, None, {}, baseline="no")
    assert set(out) == keys and torch.equal(out["loss"], -(reward * ll).mean())
    out = train.reinforce_loss(pol, None, {}, baseline="shared", num_starts=2)
    r, l2 = ea.unbatchify(reward, 2), ea.unbatchify(ll, 2)
    assert set(out) == keys and torch.equal(out["loss"], -((r - r.mean(1, keepdim=True)) * l2).mean())
    v = torch.tensor([-3.5, -4.0, -4.5, -6.0, -2.5, -6.0])
    out = train.reinforce_loss(pol, None, {}, baseline="critic", critic=lambda td: v[:, None])
    assert set(out) == keys | {"bl_val", "bl_loss"}
    assert torch.equal(out["loss"], -((reward - v) * ll).mean() + torch.nn.functional.mse_loss(v, reward))
    with pytest.raises(ValueError):           # a name that is none of the baselines no longer means "no baseline"
        train.reinforce_loss(pol, None, {}, baseline="rolout")
