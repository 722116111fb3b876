"""Development only: what the greedy-rollout baseline (eam_rl4co_amd/baselines.py: RolloutBaseline) costs at TSP-100, in one
process, wall-clock medians around a device synchronisation after warm-up, min and max beside each median:
  (a) epoch_callback on an evaluation dataset of 10 000 instances (the candidate's greedy rollouts in chunks of 1024, the copy to
      the host, the comparison of the means; the candidate is the policy the copy was made from, so the baseline is kept), and _update_policy
      (deepcopy + a fresh dataset + the copy's rollouts) on its own;
  (b) wrap_dataset on a device-resident training dataset of 20 480 instances -> instances per second;
  (c) one training step (PolicyGradientStep, batch 512) with baseline="rollout" -- `extra` given, and evaluated on the fly --
      against baseline="mean" on the parent's code path, alternately, on three policies with the same weights.
usage: time_baselines.py [out.json] [repeats]    (recorded: profiles/r13a_baselines.json)"""
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eam_rl4co_amd as ea  # noqa: E402
from eam_rl4co_amd.baselines import as_tensordict  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
WARMUP = 2
DEV = "cuda"


def timed_alternating(fns: dict, n):
    """Every function once per round, in turn: drift of the machine falls on all of them alike."""
    ms = {k: [] for k in fns}
    for i in range(WARMUP + n):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms[k].append(1e3 * (time.perf_counter() - t0))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), repeats=n) for k, v in ms.items()}


torch.manual_seed(1)
env = ea.get_env("tsp", generator_params=dict(num_loc=100))
pol = ea.AttentionModelPolicy(env_name="tsp").to(DEV).train()
res = dict(env="tsp", nodes=100, eval_instances=10_000, eval_batch=1024, train_instances=20_480, train_batch=512)

rb = ea.RolloutBaseline()
rb.setup(pol, env, batch_size=1024, dataset_size=10_000)
res.update(timed_alternating({
    "epoch_callback_keep": lambda: rb.epoch_callback(pol, env=env, batch_size=1024, epoch=0, dataset_size=10_000),
    "update_policy": lambda: rb._update_policy(pol, env, 1024, None, 10_000),
}, REPEATS))
vals = rb.bl_vals.copy()
t0 = time.perf_counter()
for _ in range(20):
    ea.paired_ttest(vals + 0.01, vals[::-1])
res["paired_ttest_10000_ms"] = 1e3 * (time.perf_counter() - t0) / 20

train_td = as_tensordict(env.dataset([20_480]), DEV)
r = timed_alternating({"wrap_dataset": lambda: rb.wrap_dataset(train_td, env, batch_size=1024)}, REPEATS)
r["wrap_dataset"]["instances_per_s"] = 20_480 / (1e-3 * r["wrap_dataset"]["median_ms"])
res.update(r)

batch = rb.wrap_dataset(train_td[:512], env, batch_size=512)
td = env.reset(batch)
steps = {}
for name, baseline in (("step_mean", "mean"), ("step_rollout_extra", "rollout"), ("step_rollout_on_the_fly", "rollout")):
    p2 = copy.deepcopy(pol)
    step = ea.PolicyGradientStep(p2, env, baseline=baseline)
    if baseline == "rollout":
        step.setup(batch_size=1024, dataset_size=1024)
        step.baseline.alpha = 1.0          # past the warm-up
    extra = batch["extra"] if name == "step_rollout_extra" else None
    steps[name] = (lambda step=step, extra=extra: step(td, extra=extra)) if baseline == "rollout" else (lambda step=step: step(td))
r = timed_alternating(steps, REPEATS)
res.update(r)
res["step_rollout_extra_minus_mean_ms"] = r["step_rollout_extra"]["median_ms"] - r["step_mean"]["median_ms"]
res["step_mean_spread_ms"] = r["step_mean"]["max_ms"] - r["step_mean"]["min_ms"]
res["step_on_the_fly_minus_extra_ms"] = r["step_rollout_on_the_fly"]["median_ms"] - r["step_rollout_extra"]["median_ms"]
print(json.dumps(res), flush=True)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
