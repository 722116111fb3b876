#!/usr/bin/env python3
"""Generate tests/golden/baselines_host.npz, baselines_structs.json and train_am_tsp20_rollout.npz by RUNNING THE REFERENCE.

    python tests/golden/make_golden_baselines.py

Same machinery as make_golden_ppo.py (reference modules through `_refshim`, closed-form `goldweights`).  The reference's
rl/reinforce/baselines.py and rl/common/utils.py are plain files and import as they are.  rl/reinforce/reinforce.py and
zoo/earl/model.py derive from a Lightning module (absent): empty stand-ins are registered for the Lightning names and for
`RL4COLitModule`, and `REINFORCE.calculate_loss` / `EAM.calculate_loss` -- the reference's own functions, unmodified -- are then
called on a plain object that carries the three attributes they read (`baseline`, `advantage_scaler`, `env`).  If the EAM
module cannot be imported that way the script says so and records only the REINFORCE cases (`has_eam` = 0).

Recorded (all float32 unless said otherwise):
  * ExponentialBaseline / MeanBaseline value sequences over 5 batches; WarmupBaseline(ExponentialBaseline-like stub) values and
    losses over 3 epochs x 2 batches with n_epochs = 2 (alpha 0, 0.5, 1);
  * calculate_loss for bl_val a scalar (warm-up at alpha 0), `extra` [B], `extra` [B, 1], a SharedBaseline on [B, S] -- from
    REINFORCE; and from EAM: [B, 1] rewards with `extra` [B], and the [2B, 1] rewards with `extra` [B] -> [2B] case, B = 4;
  * RewardScaler("norm" / "scale" / 3) over 3 batches;
  * scipy.stats.ttest_rel on float64 pairs: n = 2, n = 5, n = 64, a near-zero-variance pair, a constant difference;
  * the class structure of get_reinforce_baseline for every name (baselines_structs.json);
  * one training step of the reference AM on TSP-20 with the rollout baseline: RolloutBaseline.setup on a recorded evaluation
    dataset, wrap_dataset's values for the batch, the sampled step with recorded noise, loss and gradients as the train fixtures.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refshim  # noqa: E402,F401
import goldweights  # noqa: E402,F401
from make_golden import Recorder, gen_params, make_policy, np_  # noqa: E402

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from tensordict import TensorDict  # noqa: E402  (the stand-in of _refshim)

from rl4co.envs.routing.tsp.env import TSPEnv  # noqa: E402

_BASE = importlib.util.find_spec("rl4co").submodule_search_locations[0]


def _skip_init(pkg):
    if pkg not in sys.modules:
        m = types.ModuleType(pkg)
        m.__path__ = [_BASE + "/" + "/".join(pkg.split(".")[1:])]
        sys.modules[pkg] = m


for _pkg in ("rl4co.models.rl", "rl4co.models.rl.common", "rl4co.models.rl.reinforce", "rl4co.models.zoo.earl"):
    _skip_init(_pkg)


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _LitModule(nn.Module):
    """Stand-in of RL4COLitModule: nothing of it is executed by calculate_loss."""

    def __init__(self, env=None, policy=None, **kw):
        super().__init__()
        self.env, self.policy = env, policy

    def save_hyperparameters(self, *a, **k):
        pass


_stub("lightning", LightningModule=_LitModule)
_stub("lightning.fabric")
_stub("lightning.fabric.utilities")
_stub("lightning.fabric.utilities.types", _MAP_LOCATION_TYPE=object, _PATH=str)
_stub("lightning.pytorch")
_stub("lightning.pytorch.core")
_stub("lightning.pytorch.core.saving", _load_from_checkpoint=None)
_stub("rl4co.models.rl.common.base", RL4COLitModule=_LitModule)
_stub("rl4co.utils.lightning", get_lightning_device=lambda m: "cpu")

from rl4co.models.rl.common.utils import RewardScaler  # noqa: E402
from rl4co.models.rl.reinforce import baselines as ref_bl  # noqa: E402
from rl4co.models.rl.reinforce.reinforce import REINFORCE  # noqa: E402

try:
    _refshim.install_numba()
    _stub("torchrl.modules")                                # (SymNCO's policy, imported at the end of earl/model.py, names an MLP)
    _stub("torchrl.modules.models", MLP=nn.Module)
    from rl4co.models.zoo.am.policy import AttentionModelPolicy  # noqa: E402

    sys.modules["rl4co.models.zoo.am"].AttentionModelPolicy = AttentionModelPolicy
    from rl4co.models.zoo.earl.model import EAM  # noqa: E402
except Exception as e:  # noqa: BLE001
    print(f"EAM not importable under the shim ({type(e).__name__}: {e}): only REINFORCE.calculate_loss is pinned")
    EAM = None

torch.set_num_threads(1)


class _Holder:
    """What calculate_loss reads of `self`."""

    def __init__(self, baseline, scale=None):
        self.baseline, self.advantage_scaler, self.env = baseline, RewardScaler(scale), None


def _loss_case(fx, tag, cls, baseline, reward, ll, extra=None, scale=None):
    h = _Holder(baseline, scale)
    batch = {} if extra is None else {"extra": extra}
    out = {"reward": reward, "log_likelihood": ll}
    cls.calculate_loss(h, None, batch, out, reward, ll)
    fx[f"{tag}__reward"], fx[f"{tag}__ll"] = np_(reward), np_(ll)
    if extra is not None:
        fx[f"{tag}__extra"] = np_(extra)
    for k in ("loss", "reinforce_loss", "bl_val"):
        fx[f"{tag}__{k}"] = np_(torch.as_tensor(out[k]))
    fx[f"{tag}__bl_loss"] = np_(torch.as_tensor(out["bl_loss"], dtype=torch.float32))
    print(f"{tag}: loss={float(out['loss']):.6f} bl_val shape={tuple(torch.as_tensor(out['bl_val']).shape)}")


class _ConstBaseline(ref_bl.REINFORCEBaseline):
    """An inner baseline with a value and a loss of its own (per-row value = 2 * reward's row index, loss 0.25)."""

    def eval(self, td, reward, env=None):
        return torch.arange(reward.shape[0], dtype=reward.dtype) * 2.0, torch.tensor(0.25)


def host_fixture():
    g = torch.Generator().manual_seed(2024)
    fx = {"torch_version": np.array(torch.__version__), "has_eam": np.array(int(EAM is not None))}
    # --- exponential / mean sequences ---------------------------------------------------------------------------------
    batches = [torch.randn(6, generator=g) - 5.0 for _ in range(5)]
    fx["seq_rewards"] = np.stack([np_(b) for b in batches])
    for tag, bl in (("exp08", ref_bl.ExponentialBaseline(0.8)), ("mean", ref_bl.MeanBaseline())):
        fx[f"seq_{tag}"] = np.stack([np_(bl.eval(None, b)[0]) for b in batches])
    # --- warm-up over 3 epochs x 2 batches, n_epochs = 2 ---------------------------------------------------------------
    wb = ref_bl.WarmupBaseline(_ConstBaseline(), n_epochs=2, warmup_exp_beta=0.8)
    vals, losses, alphas = [], [], []
    for epoch in range(3):
        for b in batches[:2]:
            v, l = wb.eval(None, b)
            vals.append(np_(torch.as_tensor(v, dtype=torch.float32).expand(6)))
            losses.append(float(l))
        wb.epoch_callback(epoch=epoch)
        alphas.append(float(wb.alpha))
    fx["warmup_vals"], fx["warmup_losses"], fx["warmup_alphas"] = np.stack(vals), np.array(losses, np.float32), np.array(alphas)
    # --- calculate_loss shape cases -------------------------------------------------------------------------------------
    B = 4
    r, ll = torch.randn(B, generator=g) - 6.0, -torch.rand(B, generator=g) * 30.0
    ex = r + 0.3 * torch.randn(B, generator=g)
    warm = ref_bl.WarmupBaseline(ref_bl.RolloutBaseline())
    _loss_case(fx, "rf_scalar", REINFORCE, warm, r, ll)                                   # alpha 0: exponential, 0-dim
    _loss_case(fx, "rf_extra_b", REINFORCE, ref_bl.NoBaseline(), r, ll, extra=ex)
    _loss_case(fx, "rf_extra_b1", REINFORCE, ref_bl.NoBaseline(), r[:, None], ll[:, None], extra=ex[:, None])
    rs, lls = torch.randn(B, 3, generator=g) - 6.0, -torch.rand(B, 3, generator=g) * 30.0
    _loss_case(fx, "rf_shared", REINFORCE, ref_bl.SharedBaseline(), rs, lls)
    _loss_case(fx, "rf_norm", REINFORCE, ref_bl.NoBaseline(), r, ll, extra=ex, scale="norm")
    if EAM is not None:
        r2 = torch.cat([r, r + torch.rand(B, generator=g)])[:, None]
        ll2 = torch.cat([ll, -torch.rand(B, generator=g) * 30.0])[:, None]
        _loss_case(fx, "eam_extra_b", EAM, ref_bl.NoBaseline(), r[:, None], ll[:, None], extra=ex)
        _loss_case(fx, "eam_extra_2b", EAM, ref_bl.NoBaseline(), r2, ll2, extra=ex)     # [B] -> [2B] against [2B, 1]
        _loss_case(fx, "eam_scalar_2b", EAM, ref_bl.WarmupBaseline(ref_bl.RolloutBaseline()), r2, ll2)
        assert fx["eam_extra_2b__bl_val"].shape == (2 * B,)
    # --- RewardScaler ---------------------------------------------------------------------------------------------------
    xs = [torch.randn(5, generator=g) * 2.0 + 1.0 for _ in range(3)]
    fx["scaler_in"] = np.stack([np_(x) for x in xs])
    for scale in ("norm", "scale", 3):
        sc = RewardScaler(scale)
        fx[f"scaler_{scale}"] = np.stack([np_(sc(x.clone())) for x in xs])
    # --- ttest_rel --------------------------------------------------------------------------------------------------------
    from scipy.stats import ttest_rel

    rng = np.random.default_rng(7)
    a64 = rng.normal(-8.0, 1.0, 64)
    pairs = {"n2": (np.array([-7.5, -8.25]), np.array([-7.0, -8.0])),
             "n5": (rng.normal(-8, 1, 5), rng.normal(-8, 1, 5)),
             "n64": (a64, a64 + rng.normal(0.02, 0.1, 64)),
             "n64_far": (a64, a64 + rng.normal(0.5, 0.1, 64)),
             "tiny_var": (a64, a64 + 0.125 + 1e-9 * rng.normal(0, 1, 64)),
             "const": (a64, a64 + 0.125)}
    for k, (a, b) in pairs.items():
        with np.errstate(all="ignore"):
            t, p = ttest_rel(a, b)
        fx[f"tt_{k}__a"], fx[f"tt_{k}__b"], fx[f"tt_{k}__tp"] = a, b, np.array([t, p], np.float64)
        print(f"ttest {k}: t={t!r} p={p!r}")
    fx["tt_names"] = np.array(list(pairs))
    np.savez_compressed(os.path.join(HERE, "baselines_host.npz"), **fx)


def structures():
    def describe(b):
        d = {"class": type(b).__name__}
        for k in ("beta", "alpha", "n_epochs", "bl_alpha"):
            if hasattr(b, k):
                d[k] = getattr(b, k)
        for k in ("baseline", "warmup_baseline"):
            if isinstance(getattr(b, k, None), ref_bl.REINFORCEBaseline):
                d[k] = describe(getattr(b, k))
        if hasattr(b, "critic"):
            d["critic"] = None if b.critic is None else type(b.critic).__name__
        return d

    cases = {"no": ("no", {}), "none": (None, {}), "shared": ("shared", {}), "exponential": ("exponential", {}),
             "exponential_beta": ("exponential", {"beta": 0.5}), "mean": ("mean", {}), "critic": ("critic", {}),
             "rollout_only": ("rollout_only", {}), "rollout_only_alpha": ("rollout_only", {"bl_alpha": 0.1}),
             "rollout": ("rollout", {}), "rollout_kw": ("rollout", {"n_epochs": 3, "exp_beta": 0.6, "bl_alpha": 0.01}),
             "warmup": ("warmup", {})}
    # ("warmup" with baseline= raises TypeError in the reference: the keyword reaches WarmupBaseline twice.  Not recorded.)
    out = {k: {"name": n, "kwargs": kw, "structure": describe(ref_bl.get_reinforce_baseline(n, **kw))} for k, (n, kw) in cases.items()}
    try:
        ref_bl.get_reinforce_baseline("nonsense")
        out["unknown_raises"] = None
    except ValueError:
        out["unknown_raises"] = "ValueError"
    out["registry"] = sorted(ref_bl.REINFORCE_BASELINES_REGISTRY)
    with open(os.path.join(HERE, "baselines_structs.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("baselines_structs.json:", len(cases), "cases")


def train_fixture(name="train_am_tsp20_rollout", num_loc=20, batch=8, n_eval=16, data_seed=31, sample_seed=4321):
    """AM TSP-20, one step of REINFORCE with the rollout baseline (alpha = 1: the warm-up is over): the reference's
    RolloutBaseline is set up from the policy (deepcopy, greedy evaluation of the evaluation dataset), wraps the training batch
    (`extra` = the copy's greedy rewards) and REINFORCE.calculate_loss takes the sampled step's loss."""
    # as make_golden_ppo.py: a seed at which the recording's own float32 rounding lies within the tolerance it will be matched
    # with (biases in front of a batch norm have gradients that are pure rounding, at about the floor of that rule)
    for seed in range(data_seed, data_seed + 16):
        ratio, where = _train_fixture(name, num_loc, batch, n_eval, seed, sample_seed)
        if ratio <= OWN_ROUNDING_MAX:
            return
        print(f"{name}: data seed {seed} not used, the reference's own float32 rounding is {ratio:.2f} x the tolerance ({where})")
    raise RuntimeError(f"{name}: no data seed qualifies")


OWN_ROUNDING_MAX = 1.0


def _own_rounding(p32, p64):
    """The float32 gradients against the float64 run by the rule of tests/test_gpu_train.py:98-109 -> (worst error / bound, name)."""
    p32, p64 = dict(p32.named_parameters()), dict(p64.named_parameters())
    total = float(np.sqrt(sum(float(p.grad.double().norm()) ** 2 for p in p32.values() if p.grad is not None)))
    worst = (0.0, "")
    for k, p in p32.items():
        if p.grad is None:
            continue
        n32, g64 = float(p.grad.double().norm()), p64[k].grad
        worst = max(worst, (abs(n32 - float(g64.norm())) / (1e-4 * max(n32, 1e-3 * total) + 1e-7), f"|{k}|"))
        if p.numel() <= 512:
            bound = 1e-4 * max(float(p.grad.abs().max()), 1e-3 * total)
            worst = max(worst, (float((p.grad.double() - g64).abs().max()) / bound, k))
    return worst


def _train_fixture(name, num_loc, batch, n_eval, data_seed, sample_seed):
    import copy

    env = TSPEnv(generator_params=gen_params("tsp", num_loc), seed=data_seed)
    torch.manual_seed(data_seed)
    eval_ds = env.dataset(batch_size=[n_eval])
    train_ds = env.dataset(batch_size=[batch])
    policy = make_policy("tsp").train()
    pol64 = copy.deepcopy(policy).double()
    bl = ref_bl.RolloutBaseline()
    bl.dataset = eval_ds
    bl._update_policy(policy, env, batch_size=5, device="cpu", dataset_size=n_eval, dataset=eval_ds)
    wrapped = bl.wrap_dataset(train_ds, env, batch_size=3, device="cpu")
    b = wrapped.collate_fn([wrapped[i] for i in range(len(wrapped))])
    td = env.reset(b)
    assert policy.training                  # the greedy passes ran on the baseline's copy: the live policy still trains
    torch.manual_seed(sample_seed)
    with Recorder(policy) as rec:
        out = policy(td.clone(), env, phase="train", select_best=False, return_sum_log_likelihood=False)
    logp = out["log_likelihood"]
    out["log_likelihood"] = logp.sum(1)
    REINFORCE.calculate_loss(_Holder(bl), td, b, out)
    out["loss"].backward()
    # the same step in float64 on the same tours and baseline values: how much rounding the recorded float32 numbers carry
    td64 = TensorDict({k: (v.double() if v.is_floating_point() else v) for k, v in td.items()}, batch_size=td.batch_size)
    o64 = pol64(td64, env, phase="train", actions=out["actions"], return_sum_log_likelihood=False)
    (-((o64["reward"] - b["extra"].double()) * o64["log_likelihood"].sum(1)).mean()).backward()
    own = _own_rounding(policy, pol64)
    if own[0] > OWN_ROUNDING_MAX:
        return own
    fx = {"torch_version": np.array(torch.__version__), "env_name": np.array("tsp"), "decode_type": np.array("sampling"),
          "data_seed": np.array(data_seed), "own_rounding": np.array(own[0]),
          "baseline": np.array("rollout"), "num_starts": np.array(0, dtype=np.int64),
          "eval_locs": np_(torch.stack([d["locs"] for d in eval_ds.data])), "bl_vals": np.asarray(bl.bl_vals), "bl_mean": np.array(bl.mean),
          "locs": np_(b["locs"]), "extra": np_(b["extra"]), "actions": np_(out["actions"]), "reward": np_(out["reward"]),
          "logp_steps": np_(logp), "loss": np_(out["loss"]), "bl_val": np_(out["bl_val"]),
          "noise": np.stack([np_(q) for q in rec.noise], 1)}
    names, norms = [], []
    for k, prm in policy.named_parameters():
        g = prm.grad if prm.grad is not None else torch.zeros_like(prm)
        names.append(k)
        norms.append(float(g.double().norm()))
        if g.numel() <= 512:
            fx["grad__" + k] = np_(g)
    fx["grad_names"], fx["grad_norms"] = np.array(names), np.array(norms, dtype=np.float64)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **fx)
    print(f"{name}: loss={float(out['loss']):.6f} |grad|={np.sqrt((fx['grad_norms'] ** 2).sum()):.6f} bl mean={bl.mean:.4f} "
          f"-> {os.path.getsize(path) / 1024:.0f} KiB; data seed {data_seed}; own float32 rounding {own[0]:.2f} x the tolerance ({own[1]})")
    return own


if __name__ == "__main__":
    host_fixture()
    structures()
    train_fixture()
