"""Development only: what the logit-key-only backward buys an EAS-Emb iteration (eam_rl4co_amd/search.py), at POMO TSP-100 and
CVRP-100, 16 instances x 8 augmentations x 100 starts, in one process, HIP-event medians after warm-up:
  (a) ReevalPlan.backward_lp against ReevalPlan.backward on the same plan (the sampled rows of one iteration: the rollout's
      log-probs and heads handed in), with the run-to-run spread of each (min .. max of the repeats);
  (b) one whole EAS iteration (refresh, rollout, incumbent rows, gradient, Adam step, incumbent update) on the fast path
      against the general path.
usage: time_eas.py [out.json] [repeats]    (recorded: profiles/r08a_time_eas.json)"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eam_rl4co_amd as ea  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARMUP = 3


def timed(fn, n):
    ms = []
    for i in range(WARMUP + n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), repeats=n)


results = []
for env_name in ("tsp", "cvrp"):
    torch.manual_seed(1)
    env = ea.get_env(env_name, generator_params=dict(num_loc=100))
    pol = ea.AttentionModelPolicy(env_name=env_name, num_encoder_layers=6, normalization="instance",
                                  use_graph_context=False).eval().to("cuda")
    td = env.reset(batch_size=[16]).to("cuda")
    eas = ea.EASEmb(env, pol)
    s = eas.begin(td, seed=1)
    eas.step(s)                                            # an incumbent exists from here on
    eas._refresh(s)
    actions, logp, heads, reward = eas._rollout(s)
    plan = eas._plan(s, actions, s.S, rollout_logp=logp, rollout_heads=heads)
    g = torch.randn(actions.shape, device="cuda")
    res = dict(env=env_name, nodes=s.M, instances=s.B, augmentations=s.n_aug, starts=s.S, rows=actions.shape[0],
               steps=actions.shape[1], heads_captured=heads is not None, nchunk=plan.nchunk)
    res["backward_lp"] = timed(lambda: plan.backward_lp(g), REPEATS)
    res["backward_full"] = timed(lambda: plan.backward(g), REPEATS)
    full, lp = res["backward_full"], res["backward_lp"]
    res["backward_gain_ms"] = full["median_ms"] - lp["median_ms"]
    res["backward_full_spread_ms"] = full["max_ms"] - full["min_ms"]
    res["backward_lp_faster_than_spread"] = res["backward_gain_ms"] > res["backward_full_spread_ms"]
    for name, general in (("iteration_fast", False), ("iteration_general", True)):
        si = eas.begin(td, seed=1)
        res[name] = timed(lambda: eas.step(si, general=general), max(5, REPEATS // 2))
    results.append(res)
    print(json.dumps(res), flush=True)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
