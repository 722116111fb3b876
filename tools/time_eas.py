"""Development only: what the logit-key-only backward buys an EAS-Emb iteration (eam_rl4co_amd/search.py), at POMO TSP-100 and
CVRP-100, 16 instances x 8 augmentations x 100 starts, in one process, HIP-event medians after warm-up:
  (a) ReevalPlan.backward_lp against ReevalPlan.backward on the same plan (the sampled rows of one iteration: the rollout's
      log-probs and heads handed in), with the run-to-run spread of each (min .. max of the repeats);
  (b) one whole EAS iteration (refresh, rollout, incumbent rows, gradient, Adam step, incumbent update) on the fast path
      against the general path.
and the EAS-Lay column at the same shapes:
  (c) the layer rollout (rollout(eas_layer=), S rows per instance, pre-layer heads captured) against the plain seeded rollout of
      the same rows with the same capture, each on a state prepared outside the timed region;
  (d) ReevalPlan.backward_layer against ReevalPlan.backward_lp on the same plan (the layer rollout's log-probs and heads);
  (e) one whole EASLay iteration (rollout of S + 1 rows, one backward_layer launch, Adam step, incumbent update) against one
      whole EASEmb fast-path iteration.
usage: time_eas.py [out.json] [repeats]    (recorded: profiles/r08a_time_eas.json; profiles/r13a_time_eas_lay.json)"""
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
    # ---- EAS-Lay ----
    from eam_rl4co_amd import ops
    from eam_rl4co_amd.policy import _env_step_, _max_decode_steps, state_from_td

    lay = ea.EASLay(env, pol)
    sl = lay.begin(td, seed=1)
    lay.step(sl)
    lay.step(sl)                                           # W2 has moved, an incumbent exists
    start = env.select_start_nodes(sl.td, num_starts=sl.S).to(torch.int64).contiguous()
    t_max = int(max(1, _max_decode_steps(pol.env_name, sl.M, 1)))

    def states(n):
        out = []
        for _ in range(n):
            st = state_from_td(pol.env_name, sl.td, sl.S)
            _env_step_(st, start)
            out.append(st)
        return out

    def rollouts(layer, n):
        pool = states(WARMUP + n)
        kw = dict(clip=pol.tanh_clipping, temp=pol.temperature, t_max=t_max, seed=11, want_heads=True)
        return timed(lambda: ops.rollout(pool.pop(), sl.cache, "sampling", eas_layer=layer, **kw), n)

    el = dict(rows=start.numel(), t_max=t_max)
    el["rollout_layer"] = rollouts(lay._layer_operands(sl), max(5, REPEATS // 2))
    el["rollout_plain"] = rollouts(None, max(5, REPEATS // 2))
    el["rollout_ratio"] = el["rollout_layer"]["median_ms"] / el["rollout_plain"]["median_ms"]
    la, ll, lh, _, S1 = lay._rollout_layer(sl)
    lplan = lay._plan(sl, la, S1, rollout_logp=ll, rollout_heads=lh)
    lg = torch.randn(la.shape, device="cuda")
    el["plan_rows"], el["plan_steps"], el["plan_nchunk"] = la.shape[0], la.shape[1], lplan.nchunk
    el["backward_layer"] = timed(lambda: lplan.backward_layer(lg, lay._layer_operands(sl)), REPEATS)
    el["backward_lp_same_plan"] = timed(lambda: lplan.backward_lp(lg), REPEATS)
    el["backward_ratio"] = el["backward_layer"]["median_ms"] / el["backward_lp_same_plan"]["median_ms"]
    si = lay.begin(td, seed=1)
    el["iteration_lay"] = timed(lambda: lay.step(si), max(5, REPEATS // 2))
    el["iteration_ratio_to_emb_fast"] = el["iteration_lay"]["median_ms"] / res["iteration_fast"]["median_ms"]
    res["eas_lay"] = el
    results.append(res)
    print(json.dumps(res), flush=True)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
