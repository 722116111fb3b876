"""REINFORCE baselines of the reference (rl4co/models/rl/reinforce/baselines.py:19-311): names, constructor arguments, defaults
and return shapes are the reference's.  `eval(td, reward, env)` -> (bl_val, bl_loss); `train.reinforce_loss`,
`train.eam_am_loss` and `train.PolicyGradientStep` take these objects (or their registry names) as `baseline=`.

The one baseline with a hot path is `RolloutBaseline` (Kool's greedy rollout): dataset-scale greedy rollouts of a frozen copy
of the policy.  They are this library's rollout, `policy(td, env, decode_type="greedy")` under torch.no_grad(), on chunks of one
device-resident TensorDict -- nothing here computes anything a kernel already computes.  What runs on the host is
the decision of an epoch: the paired t-test over the two reward vectors, copied once per epoch, in float64 (`paired_ttest`).

Deviations from the reference, all stated in DESIGN.md 13:
  * `RolloutBaseline.rollout` restores the policy's train / eval mode (the reference leaves the live policy in eval());
  * it runs under no_grad, not inference_mode (the live policy's cached packed weights must serve the next autograd step);
  * `RolloutBaseline.eval` decodes greedily (the reference's call takes the policy's train decode type, i.e. it samples);
  * datasets stay on the device as one TensorDict; `device=None` means the policy's device;
  * with more than one rank, rank 0's verdict of the t-test is broadcast: all ranks update the baseline or none does.
"""
from __future__ import annotations

import copy
import logging
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .critic import CriticNetwork, create_critic_from_actor
from .tensordict_lite import TensorDict

log = logging.getLogger(__name__)


# ------------------------------------------------------------------------------------------------------------
# paired t-test (scipy.stats.ttest_rel(a, b) -> statistic, two-sided p) without SciPy
# ------------------------------------------------------------------------------------------------------------
def _betacf(a: float, b: float, x: float) -> float:
    """Continued fraction of the incomplete beta function (modified Lentz), float64."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = 1.0
    d = 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 100_000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h


def _betainc(a: float, b: float, x: float) -> float:
    """Regularised incomplete beta function I_x(a, b)."""
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    lbt = math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x)
    if x < (a + 1.0) / (a + b + 2.0):
        return math.exp(lbt) * _betacf(a, b, x) / a
    return 1.0 - math.exp(lbt) * _betacf(b, a, 1.0 - x) / b


def paired_ttest(a, b):
    """The t-test on two related samples, scipy.stats.ttest_rel(a, b): -> (t, two-sided p) as Python floats.  Computed in
    float64 on the host: d = a - b, t = mean(d) / sqrt(var(d, ddof=1) / n), p = I_{df / (df + t^2)}(df / 2, 1 / 2) with
    df = n - 1.  n < 2 or d == 0 everywhere: (nan, nan); a constant non-zero d: (+-inf, 0), as SciPy returns them."""
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64).reshape(-1)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64).reshape(-1)
    if a.shape != b.shape:
        raise ValueError(f"paired_ttest: unequal lengths {a.shape[0]} and {b.shape[0]}")
    n = a.shape[0]
    if n < 2:
        return float("nan"), float("nan")
    d = a - b
    dm = float(d.mean())
    denom = math.sqrt(float(d.var(ddof=1)) / n)
    if denom == 0.0:
        if dm == 0.0:
            return float("nan"), float("nan")
        return math.copysign(float("inf"), dm), 0.0
    t = dm / denom
    df = n - 1.0
    if math.isinf(t):
        return t, 0.0
    # (t * t may overflow to inf for a near-constant d: x -> 0, p -> 0)
    t2 = t * t
    x = df / (df + t2) if not math.isinf(t2) else 0.0
    return t, _betainc(0.5 * df, 0.5, x)


# ------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------
def _is_tensordict(x) -> bool:
    return hasattr(x, "batch_size") and hasattr(x, "keys")


def _policy_device(policy):
    first = next(iter(policy.parameters()), None)
    return torch.device("cpu") if first is None else first.device


def as_tensordict(dataset, device=None):
    """A TensorDict, or a dataset that was built from one (`.td`), or any dataset with `collate_fn` -> ONE TensorDict on `device`."""
    if _is_tensordict(dataset):
        td = dataset
    elif getattr(dataset, "td", None) is not None:
        td = dataset.td
    else:
        td = dataset.collate_fn([dataset[i] for i in range(len(dataset))])
    if device is not None and td.device != torch.device(device):
        td = td.to(device)
    return td


def _world_size() -> int:
    import torch.distributed as dist

    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


# ------------------------------------------------------------------------------------------------------------
# the baselines
# ------------------------------------------------------------------------------------------------------------
class REINFORCEBaseline(nn.Module):
    """What a REINFORCE trainer asks of a baseline.  `eval(td, reward, env)` returns the pair (value subtracted from the reward,
    loss term added to the policy's loss).  The three hooks do nothing unless a baseline needs them: `setup` once before
    training, `wrap_dataset` on every epoch's training dataset, `epoch_callback` after every epoch."""

    def __init__(self, *args, **kw):
        super().__init__()

    def eval(self, td, reward, env=None, **kwargs):
        raise NotImplementedError(f"{type(self).__name__}.eval")

    def setup(self, *args, **kw):
        return None

    def wrap_dataset(self, dataset, *args, **kw):
        return dataset

    def epoch_callback(self, *args, **kw):
        return None


class NoBaseline(REINFORCEBaseline):
    """Plain REINFORCE: nothing is subtracted, nothing is added."""

    def eval(self, td, reward, env=None):
        return 0, 0


class SharedBaseline(REINFORCEBaseline):
    """POMO's baseline: rewards arrive as [B, S]; each instance's value is the mean over its S rollouts, kept as [B, 1]."""

    def eval(self, td, reward, env=None, on_dim=1):
        return reward.mean(dim=on_dim, keepdims=True), 0


class ExponentialBaseline(REINFORCEBaseline):
    """One scalar for the whole batch: a moving average of the batches' mean rewards in which the past weighs `beta`.
    The first batch sets it.  `v` holds the current value (a 0-dim tensor without a graph)."""

    def __init__(self, beta=0.8, **kw):
        super().__init__()
        self.beta = beta
        self.v = None

    def eval(self, td, reward, env=None):
        batch_mean = reward.detach().mean()
        self.v = batch_mean if self.v is None else self.beta * self.v + (1.0 - self.beta) * batch_mean
        return self.v, 0


def MeanBaseline(**kw):
    """The batch mean as baseline: an `ExponentialBaseline` that forgets the past at once (beta = 0)."""
    return ExponentialBaseline(beta=0.0, **kw)


class WarmupBaseline(REINFORCEBaseline):
    """Fades from an exponential baseline (`warmup_exp_beta`) into `baseline` over the first `n_epochs` epochs.  `alpha` is the
    share of `baseline`: 0 until the first epoch has ended, (epoch + 1) / n_epochs after epoch `epoch`, 1 from then on.  Value
    and loss are mixed with the same weights.  At alpha 0 only the exponential baseline is evaluated, at 1 only `baseline`."""

    def __init__(self, baseline, n_epochs=1, warmup_exp_beta=0.8, **kw):
        super().__init__()
        assert n_epochs > 0, "n_epochs to warmup must be positive"
        self.baseline = baseline
        self.warmup_baseline = ExponentialBaseline(warmup_exp_beta)
        self.n_epochs = n_epochs
        self.alpha = 0

    def setup(self, *args, **kw):
        self.baseline.setup(*args, **kw)

    def wrap_dataset(self, dataset, *args, **kw):
        # the inner baseline's values are of no use before it has any weight
        target = self.baseline if self.alpha > 0 else self.warmup_baseline
        return target.wrap_dataset(dataset, *args, **kw)

    def eval(self, td, reward, env=None):
        a = self.alpha
        if a <= 0:
            return self.warmup_baseline.eval(td, reward, env)
        if a >= 1:
            return self.baseline.eval(td, reward, env)
        inner, warm = self.baseline.eval(td, reward, env), self.warmup_baseline.eval(td, reward, env)
        return tuple(a * x + (1 - a) * y for x, y in zip(inner, warm))

    def epoch_callback(self, *args, **kw):
        self.baseline.epoch_callback(*args, **kw)           # every epoch: the rollout baseline is challenged during the warm-up too
        epoch = kw["epoch"]
        if epoch < self.n_epochs:
            self.alpha = (epoch + 1) / float(self.n_epochs)
            log.info("warm-up: the baseline's share is now %s", self.alpha)


class CriticBaseline(REINFORCEBaseline):
    """A learned value: `critic(td)` [B, 1] -> value [B] (detached: the actor does not learn through it) and the critic's own
    regression loss against the reward.  Without a critic, `setup` builds one from the policy's encoder."""

    def __init__(self, critic: CriticNetwork = None, **unused_kw):
        super().__init__()
        self.critic = critic

    def setup(self, policy, env, **kwargs):
        if self.critic is not None:
            return
        log.info("CriticBaseline: no critic given, building one from the policy (%s)", getattr(env, "name", env))
        self.critic = create_critic_from_actor(policy)

    def eval(self, td, reward, env=None):
        value = self.critic(td).squeeze(-1)
        return value.detach(), F.mse_loss(value, reward.detach())


class RolloutBaseline(REINFORCEBaseline):
    """Kool's greedy-rollout baseline: the value of an instance is the greedy reward of a frozen copy of the policy.  After every
    epoch the live policy is compared with the copy on the evaluation dataset; where its mean reward is higher and a paired
    t-test gives one-sided p < `bl_alpha`, the copy is replaced by the live policy and a new evaluation dataset is drawn.

    State: `policy` (the copy: eval mode, no gradients), `dataset` (ONE TensorDict on the device, generator output before
    reset; not pickled), `bl_vals` (the copy's rewards on it: float64 on the host; `bl_vals_device`: float32 on the device) and
    `mean`.  The evaluation dataset needs at least two instances."""

    def __init__(self, bl_alpha=0.05, **kw):
        super().__init__()
        self.bl_alpha = bl_alpha
        self.dataset = None

    # ---- the copy ------------------------------------------------------------------------------------------------
    def setup(self, *args, **kw):
        self._update_policy(*args, **kw)

    def _update_policy(self, policy, env, batch_size=64, device=None, dataset_size=None, dataset=None):
        """Take a frozen copy of `policy` and evaluate it on `dataset`, or on a new one of `dataset_size` instances
        (`env.dataset([dataset_size])`); one of the two is required."""
        device = _policy_device(policy) if device is None else torch.device(device)
        if dataset is None:
            if dataset_size is None or int(dataset_size) < 2:
                raise ValueError(f"RolloutBaseline: dataset_size={dataset_size!r}; the evaluation dataset needs at least 2 instances "
                                 "(pass dataset_size=, i.e. val_data_size, or dataset=)")
            dataset = env.dataset(batch_size=[int(dataset_size)])
        frozen = copy.deepcopy(policy).to(device).eval()
        # not part of the model: the trainer's flat gradient buffer and an open shared-graph slot.  (The copy's weight caches are
        # keyed on the address and version of the ORIGINAL parameters, so the copy never hits them and packs its own.)
        frozen.__dict__.pop("_flat_grads", None)
        frozen.__dict__.pop("_shared_dt", None)
        for p in frozen.parameters():
            p.requires_grad_(False)
        self.policy = frozen
        self.dataset = as_tensordict(dataset, device)
        if self.dataset.batch_size[0] < 2:
            raise ValueError("RolloutBaseline: the evaluation dataset needs at least 2 instances")
        self.bl_vals_device = self.rollout(frozen, env, batch_size, device, self.dataset)
        self.bl_vals = self.bl_vals_device.cpu().numpy().astype(np.float64)        # the one copy to the host
        self.mean = float(self.bl_vals.mean())
        log.info("rollout baseline: mean greedy reward %.4f on %d instances", self.mean, self.bl_vals.shape[0])

    # ---- values --------------------------------------------------------------------------------------------------
    def rollout(self, policy, env, batch_size=64, device=None, dataset=None):
        """Greedy rollouts of `policy` over `dataset` (default: the evaluation dataset) in chunks of `batch_size` -> rewards [n],
        float32, on the device.  Runs under no_grad and leaves the policy in the train / eval mode it came in."""
        if dataset is None:
            dataset = self.dataset
        if dataset is None:
            raise RuntimeError("RolloutBaseline: no evaluation dataset (it is not pickled: call setup() after loading)")
        device = _policy_device(policy) if device is None else torch.device(device)
        data = as_tensordict(dataset, device)
        mode = policy.training
        policy.eval()
        chunks = []
        try:
            with torch.no_grad():
                for lo in range(0, data.batch_size[0], batch_size):
                    td = env.reset(data[lo:lo + batch_size])
                    chunks.append(policy(td, env, decode_type="greedy")["reward"])
        finally:
            policy.train(mode)
        return torch.cat(chunks, 0)

    def eval(self, td, reward, env):
        """The copy's greedy reward on `td` [B], computed now.  `wrap_dataset` computes the same numbers once per epoch at the
        evaluation batch size; a trainer then passes them as `extra` and this is not called."""
        with torch.no_grad():
            return self.policy(td, env, decode_type="greedy")["reward"], 0

    def wrap_dataset(self, dataset, env, batch_size=64, device=None, **kw):
        """`dataset` plus the copy's greedy rewards under "extra".  A TensorDict comes back as a TensorDict, a
        TensorDictDataset through its `add_key`; the values go where the dataset's tensors are."""
        values = self.rollout(self.policy, env, batch_size, device, dataset=dataset)
        if _is_tensordict(dataset):
            return TensorDict({**dict(dataset.items()), "extra": values.to(dataset.device)}, batch_size=dataset.batch_size)
        home = as_tensordict(dataset).device if len(dataset) else values.device
        return dataset.add_key("extra", values.to(home))

    # ---- the end of an epoch ---------------------------------------------------------------------------------------
    def _beats_baseline(self, candidate_vals) -> bool:
        """Host arithmetic on the two reward vectors: is the candidate's mean higher, and significantly so?"""
        if not float(candidate_vals.mean()) - self.mean > 0:
            return False
        # paired differences baseline - candidate: negative on average here, so t < 0 (-inf where they are constant)
        t, p_two_sided = paired_ttest(self.bl_vals, candidate_vals)
        if math.isnan(t):
            raise ValueError("RolloutBaseline: the t-test is undefined on this evaluation dataset (fewer than 2 instances?)")
        return 0.5 * p_two_sided < self.bl_alpha

    def epoch_callback(self, policy, env, batch_size=64, device=None, epoch=None, dataset_size=None):
        """Evaluate the live policy on the evaluation dataset and replace the copy if it is significantly better.  With several
        ranks every rank evaluates, rank 0 decides for all.  -> whether the copy was replaced."""
        candidate_vals = self.rollout(policy, env, batch_size, device).cpu().numpy().astype(np.float64)
        replace = self._beats_baseline(candidate_vals)
        log.info("rollout baseline: candidate %.4f against %.4f -> %s", float(candidate_vals.mean()), self.mean,
                 "replace" if replace else "keep")
        if _world_size() > 1:
            import torch.distributed as dist

            where = _policy_device(policy) if dist.get_backend() == "nccl" else "cpu"
            verdict = torch.tensor([int(replace)], dtype=torch.int64, device=where)
            dist.broadcast(verdict, src=0)
            replace = bool(verdict.item())
        if replace:
            self._update_policy(policy, env, batch_size, device, dataset_size)
        return replace

    # ---- pickling: everything but the dataset ------------------------------------------------------------------------
    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k != "dataset"}

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__["dataset"] = None


REINFORCE_BASELINES_REGISTRY = {
    "no": NoBaseline, "mean": MeanBaseline, "exponential": ExponentialBaseline, "shared": SharedBaseline,
    "critic": CriticBaseline, "rollout_only": RolloutBaseline, "warmup": WarmupBaseline,
}


def get_reinforce_baseline(name, **kw):
    """A baseline by name: the registry's names, None (= "no"), and two compositions.  "rollout": the greedy rollout inside a
    warm-up, from the options `n_epochs` (1), `exp_beta` (0.8) and `bl_alpha` (0.05).  "warmup": a warm-up around `baseline=`
    (a name or an object; default "rollout"), the other options going to both.  Unknown names raise ValueError."""
    if name is None:
        name = "no"
    if name == "rollout":
        inner = RolloutBaseline(bl_alpha=kw.get("bl_alpha", 0.05))
        return WarmupBaseline(inner, n_epochs=kw.get("n_epochs", 1), warmup_exp_beta=kw.get("exp_beta", 0.8))
    if name == "warmup":
        options = dict(kw)
        inner = options.pop("baseline", "rollout")
        if not isinstance(inner, REINFORCEBaseline):
            inner = get_reinforce_baseline(inner, **options)
        return WarmupBaseline(inner, **options)
    try:
        factory = REINFORCE_BASELINES_REGISTRY[name]
    except (KeyError, TypeError):
        known = sorted(REINFORCE_BASELINES_REGISTRY) + ["rollout"]
        raise ValueError(f"get_reinforce_baseline: no baseline is called {name!r}; known: {known}") from None
    return factory(**kw)


# ------------------------------------------------------------------------------------------------------------
# advantage scaling
# ------------------------------------------------------------------------------------------------------------
class RewardScaler:
    """Scales the advantage by statistics gathered over all batches seen so far.  scale: None -> unchanged; an int -> divided
    by it; "norm" -> (x - mean) / (std + eps); "scale" -> x / (std + eps), with the running mean and the unbiased running
    standard deviation, eps the machine epsilon of x's dtype.  The statistics (`count`, `mean`, `M2` = sum of squared deviations)
    are float64 tensors on x's device, merged batch by batch with the pairwise update of Chan et al.; nothing syncs."""

    MODES = ("norm", "scale")

    def __init__(self, scale: str = None):
        self.scale = scale
        self.count = 0
        self.mean = 0.0
        self.M2 = 0.0

    @torch.no_grad()
    def update(self, batch: torch.Tensor):
        x = batch.detach().reshape(-1).double()
        n = x.numel()
        if n == 0:
            return
        batch_mean = x.mean()
        total = self.count + n
        shift = batch_mean - self.mean
        self.M2 = self.M2 + (x - batch_mean).square().sum() + shift * shift * (self.count * n / total)
        self.mean = self.mean + shift * (n / total)
        self.count = total

    def __call__(self, scores: torch.Tensor):
        mode = self.scale
        if mode is None:
            return scores
        if isinstance(mode, int):
            return scores / mode
        if mode not in self.MODES:
            raise ValueError(f"RewardScaler: scale must be None, an int, 'norm' or 'scale', got {mode!r}")
        self.update(scores)
        std = torch.sqrt(self.M2 / (self.count - 1)).to(scores.dtype)
        centre = self.mean.to(scores.dtype) if mode == "norm" else 0
        return (scores - centre) / (std + torch.finfo(scores.dtype).eps)
