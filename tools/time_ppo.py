"""Development only: what the entropy term costs the re-evaluation backward and what the native path buys a PPO step
(eam_rl4co_amd/train.py: PPOStep), at TSP-100 x 512 and CVRP-100 x 512 with mini_batch_size = 0.25 (mini-batches of 128), in
one process, HIP-event medians after warm-up, min and max beside each median:
  (a) ReevalPlan.backward(glogp, gent) against the same plan's backward(glogp) -- the kernels of the parent path; the two are
      timed alternately, at the PPO mini-batch (128 rows) and at the whole batch (512 rows);
  (b) one PPOStep (rollout + ppo_epochs x 4 mini-batches of forward, backward, clip, Adam) on the native path against
      EAMRL_NATIVE_REEVAL=0 (the PyTorch re-evaluation), alternately, on two policies with the same weights.
usage: time_ppo.py [out.json] [repeats]    (recorded: profiles/r12a_time_ppo.json)"""
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eam_rl4co_amd as ea  # noqa: E402
from eam_rl4co_amd import ops, train  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARMUP = 3


def timed_alternating(fns: dict, n):
    """Every function once per round, in turn: drift of the machine falls on all of them alike."""
    ms = {k: [] for k in fns}
    for i in range(WARMUP + n):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms[k].append(e0.elapsed_time(e1))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), repeats=n) for k, v in ms.items()}


def plan_for(pol, env, td, actions):
    """The plan `train._evaluate_native` builds for these tours, with the entropy output."""
    with torch.no_grad():
        t = train.decoder_tensors(pol, td)
        E = t["emb"].shape[-1]
        Wctx = t["Wctx"]
        parts = [t["K"], t["V"], t["L"] @ t["Wout"], t["emb"] @ Wctx[:, :E].t()]
        if pol.env_name == "tsp":
            parts.append(t["emb"] @ Wctx[:, E:2 * E].t())
        meta = train.replay_states(pol, td, actions, 1, False)
        if pol.env_name == "tsp":
            cvec = (t["placeholder"][None] @ Wctx.t()) if meta["placeholder"] else None
        else:
            cvec = Wctx[:, E:].t().contiguous()
        buf = torch.cat(parts, -1).contiguous()
        return ops.ReevalPlan(buf, pol.env_name == "tsp", t.get("gctx"), cvec, meta["idxA"], meta["idxB"], meta["sc"],
                              meta["maskbits"], actions.contiguous(), 1, meta["tstart"], float(pol.tanh_clipping),
                              float(pol.temperature), want_entropy=True)


results = []
for env_name in ("tsp", "cvrp"):
    torch.manual_seed(1)
    env = ea.get_env(env_name, generator_params=dict(num_loc=100))
    pol = ea.AttentionModelPolicy(env_name=env_name).to("cuda").train()
    td = env.reset(batch_size=[512]).to("cuda")
    with torch.no_grad():
        actions = pol(td.clone(), env, phase="train")["actions"].contiguous()
    res = dict(env=env_name, nodes=td["locs"].shape[1], instances=512, steps=actions.shape[1], mini_batch=128)
    # (a) the backward with and without the entropy gradient
    for tag, rows in (("mini_batch_128", 128), ("batch_512", 512)):
        idx = torch.arange(rows)
        plan = plan_for(pol, env, td[idx], actions[:rows])
        plan.forward()
        g = torch.randn(actions[:rows].shape, device="cuda")
        ge = torch.full_like(g, -0.01 / rows)
        r = timed_alternating({"backward": lambda: plan.backward(g), "backward_gent": lambda: plan.backward(g, ge)}, REPEATS)
        r["entropy_term_ms"] = r["backward_gent"]["median_ms"] - r["backward"]["median_ms"]
        r["backward_spread_ms"] = r["backward"]["max_ms"] - r["backward"]["min_ms"]
        r["entropy_term_above_spread"] = r["entropy_term_ms"] > r["backward_spread_ms"]
        r["nchunk"] = plan.nchunk
        res["reeval_" + tag] = r
    # (b) one PPO step, native re-evaluation against the PyTorch path
    steps = {}
    for name, native in (("ppo_step_native", "1"), ("ppo_step_pytorch", "0")):
        p2 = copy.deepcopy(pol)
        step = ea.PPOStep(p2, env, mini_batch_size=0.25, entropy_lambda=0.01, generator=torch.Generator().manual_seed(1))

        def run(step=step, native=native):
            os.environ["EAMRL_NATIVE_REEVAL"] = native
            try:
                return step(td)
            finally:
                os.environ.pop("EAMRL_NATIVE_REEVAL", None)

        steps[name] = run
    r = timed_alternating(steps, max(5, REPEATS // 2))
    res.update(r)
    res["ppo_step_gain_ms"] = r["ppo_step_pytorch"]["median_ms"] - r["ppo_step_native"]["median_ms"]
    results.append(res)
    print(json.dumps(res), flush=True)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
