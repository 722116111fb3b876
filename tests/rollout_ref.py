"""The yardstick of the rollout kernels' decode arithmetic: the base decode step of include/eamrl.h (eamrl_cache, eamrl_state,
eamrl_am_decode_step) along a whole rollout, as a thin layer over tests/step_ref.py (the env rule) and tests/reeval_ref.py
(query -> masked 8-head glimpse -> logits -> tanh clip -> mask -> / temperature -> log-softmax).

Written from the header and the reference's context embeddings (models/nn/env_embeddings/context.py), not from the kernels.
The query of row r (instance r % B) in the state before a step, with P = the halves of project_context folded into the node
embeddings (Pa, Pb), cvec = its state columns and gctx the graph context:

    tsp     Pa[first] + Pb[cur] + gctx; at i == 0 project_context(W_placeholder) + gctx = cvec + gctx           context.py:118-140
    cvrp    Pa[cur] + (vehicle_capacity - used_capacity) cvec + gctx                                             context.py:155-157
    sdvrp   as cvrp; row n of K / V / Lp gains rem[n] * (wk | wv | lw), rem[depot] = 0                           dynamic.py:72-78
    cvrptw  Pa[cur] + (vehicle_capacity - used_capacity) cvec[0] + current_time cvec[1] + gctx                   context.py:173-176
    pctsp   Pa[cur] + max(prize_required - cur_total_prize, 0) cvec + gctx                                       context.py:204-208
    op      Pa[cur] + (max_length[:, 0] - tour_length) cvec + gctx                                               context.py:221-223
    pdp     Pa[cur] + gctx                                                                                       context.py:251-253

A state column is the reference's own float32 difference (one float32 subtraction of two float32 state values); everything
after it is computed in the dtype of the cache: float64 is the reference, the float32 run gives the scale of float32 rounding.

`operands_of` turns a rollout's actions into the operands of reeval_ref.reeval; `run` adds the full log-prob vectors; `keys64`
is the selection key; `rollout` is the decode loop on the restatement itself (the stand-in for a kernel on the CPU).
`mutant` selects a deliberately wrong one-line variant (tests/test_host_rollout_ref.py shows that the case table sees each).

The PolyNet pointer (`poly`, an argument of `run` and `rollout`, or the entry "poly" of the cache dict): the logits are formed
from reeval_ref's heads as include/eamrl.h (eamrl_polynet) and the reference's nn/attention.py:519-556 define them,
    g = heads Wout^T;  h = relu(W1[:, :E] g + W1[:, E:] z_j + b1);  y = g + (W2 h + b2);  u[n] = y . L[n] / sqrt(E)
with L the UNFOLDED logit key (the entry "L" of the cache dict; the fold Lp = L Wout does not cover y) and z_j row
j = (s_first + r // B) % k of the strategy table.  poly: dict of Wout [E, E], W1 [P, E + dz], b1 [P], W2 [E, P], b2 [E],
Z [k, dz] (float32 tensors; everything after them is computed in the dtype of the run) and s_first (absent: 0).  Its own one-line
mutants are POLY_MUTANTS (tests/test_host_polynet_arith.py shows that tests/polynet_cases.py sees each).
One of reeval_ref's does not carry over: `rem_of_previous_step` changes nothing that a rollout can show.  A delivery either
empties its node, which is masked from then on, or fills the vehicle, after which the depot is the only feasible node and the
step after that starts from the depot with the same remaining demands; so the stale row only ever belongs to an infeasible node
or to a forced step.  `rem_of_reset` (the demands are never updated) stands in for it: a split delivery shows it.
"""
import math

import numpy as np
import torch

import reeval_ref as rr
import step_ref

E = rr.E
f32 = np.float32
REEVAL_MUTANTS = ("glimpse_unmasked", "instance_r_div_S")                  # reeval_ref's own, passed through
OPERAND_MUTANTS = ("rem_of_previous_step", "rem_of_reset", "state_column_dropped", "state_column_of_previous_step", "placeholder_ignored",
                   "first_and_current_swapped")
LOGIT_MUTANTS = ("temperature_before_clip", "mask_before_clip")
SELECT_MUTANTS = ("sampling_minus_noise", "tie_to_higher_index")
MUTANTS = REEVAL_MUTANTS + OPERAND_MUTANTS + LOGIT_MUTANTS + SELECT_MUTANTS
POLY_MUTANTS = ("strategy_of_r_mod_k", "s_first_ignored", "relu_dropped", "residual_g_dropped", "b2_dropped", "ctab_of_strategy_0",
                "folded_Lp_for_L", "padded_slots_not_zero")                 # of the PolyNet pointer (run(..., poly=))
LAUNCH_ROWS = 128           # rows of an instance per launch of the kernel: what `s_first_ignored` restarts the strategies at
N_STATE_COLS = {"tsp": 1, "cvrp": 1, "sdvrp": 1, "pctsp": 1, "spctsp": 1, "op": 1, "cvrptw": 2, "pdp": 0}    # rows of cvec


def state_columns(env, s):
    """The planes of `sc` of one row of a depot env in state s."""
    if env == "pdp":
        return []
    free = f32(s["vcap"] - s["used"])
    if env in ("pctsp", "spctsp"):
        free = max(free, f32(0.0))
    return [free, s["time"]] if env == "cvrptw" else [free]


def step_operands(env, states, prev=None, mutant=None):
    """The per-step operands of the R rows in `states` (`prev`: their states one step earlier, read by the mutants only)
    -> dict of mask [R, M] bool, idxA, idxB [R] (idxB None without a Pb plane), sc [NC, R], rem [R, M] or None."""
    prev = states if prev is None else prev
    R = len(states)
    mask = np.stack([s["mask"] for s in states])
    cur = np.array([s["cur"] for s in states], np.int32)
    idxB = None
    if env == "tsp":
        first = np.array([s["first"] for s in states], np.int32)
        fresh = np.array([s["istep"] == 0 for s in states])
        if mutant == "placeholder_ignored":
            fresh[:] = False
        idxA, idxB = (cur, first) if mutant == "first_and_current_swapped" else (first, cur)
        idxA, idxB = np.where(fresh, -1, idxA).astype(np.int32), np.where(fresh, -1, idxB).astype(np.int32)
        sc = fresh.astype(f32)[None]
    else:
        idxA = cur
        src = prev if mutant == "state_column_of_previous_step" else states
        sc = np.array([state_columns(env, s) for s in src], f32).reshape(R, N_STATE_COLS[env]).T.copy()
        if mutant == "state_column_dropped" and len(sc):
            sc[-1] = 0
    rem = None
    if env == "sdvrp":
        rem = np.stack([s["rem"] for s in (prev if mutant == "rem_of_previous_step" else states)]).astype(f32)
        if mutant == "rem_of_reset":
            rem = np.stack([np.concatenate([np.zeros(1, f32), s["demand"]]) for s in states])
    return dict(mask=mask, idxA=idxA, idxB=idxB, sc=sc, rem=rem)


def _assemble(cache, per_step, actions, S, tstart, clip, temp):
    """reeval_ref's operand dict from the per-step operands (a list over t) and the cache tensors."""
    st = lambda k: np.stack([p[k] for p in per_step], 1)              # [R, T, ...]
    op = {k: cache.get(k) for k in ("K", "V", "Lp", "Pa", "Pb", "gctx", "Cvec", "dyn")}
    op.update({k: cache[k] for k in ("L", "poly") if cache.get(k) is not None})         # the PolyNet pointer's, where there is one
    op.update(mask=torch.from_numpy(st("mask")), idxA=torch.from_numpy(st("idxA")), actions=torch.from_numpy(np.asarray(actions, np.int64)),
              idxB=torch.from_numpy(st("idxB")) if per_step[0]["idxB"] is not None else None,
              sc=torch.from_numpy(np.stack([p["sc"] for p in per_step], 2)) if op["Cvec"] is not None else None,
              rem=torch.from_numpy(st("rem")) if per_step[0]["rem"] is not None else None,
              S=S, tstart=tstart, clip=clip, temp=temp, heads=None)
    if op["idxB"] is None:
        op["Pb"] = None
    return op


def operands_of(cache, batch, actions, S, tstart=0, clip=10.0, temp=1.0, mutant=None, start_state=None):
    """The operands of reeval_ref.reeval along the rollout `actions` [R, T] of the R = S * B rows (row r: instance r % B), from
    the states before every step as step_ref.replay gives them.  cache: dict of K, V, Lp, Pa [B, M, E], Pb or None, gctx [B, E],
    Cvec [NC, E] or None, dyn [3, E] or None.  The dict also carries `done` [R, T] (the row was done before the step) and
    `feasible` [R, T] (the action was allowed by the mask before it); neither is read by `reeval`.  start_state: the rows' states
    before the first step where they are not the reset states (step_ref.replay)."""
    env = str(batch["env"])
    actions = np.asarray(actions, np.int64)
    hist = step_ref.replay(batch, actions, S, start_state=start_state)
    T = actions.shape[1]
    per_step = [step_operands(env, hist[t], hist[max(t - 1, 0)], mutant) for t in range(T)]
    op = _assemble(cache, per_step, actions, S, tstart, clip, temp)
    op["done"] = torch.from_numpy(np.array([[bool(s["done"]) for s in hist[t]] for t in range(T)]).T.copy())
    op["feasible"] = op["mask"].gather(2, op["actions"][..., None]).squeeze(-1)
    op["all_done"] = all(bool(s["done"]) for s in hist[T])
    return op


def polynet_y(heads, poly, B, mutant=None):
    """y [R, T, E] of the PolyNet pointer from the glimpse outputs heads [R, T, E] (row r: strategy (s_first + r // B) % k), in
    the dtype of `heads`; also the hidden pre-activations [R, T, P]."""
    w = {n: poly[n].to(heads.dtype) for n in ("Wout", "W1", "b1", "W2", "b2", "Z")}
    R = heads.shape[0]
    k, s_first = w["Z"].shape[0], int(poly.get("s_first", 0))
    s = torch.arange(R) // B
    j = (s_first + s) % k
    if mutant == "strategy_of_r_mod_k":
        j = (s_first + torch.arange(R)) % k
    elif mutant == "s_first_ignored":           # every launch of LAUNCH_ROWS rows per instance starts at strategy 0 again
        j = (s % LAUNCH_ROWS) % k
    elif mutant == "ctab_of_strategy_0":
        j = torch.zeros_like(j)
    g = heads @ w["Wout"].T
    ctab = w["Z"] @ w["W1"][:, E:].T + w["b1"]                                  # [k, P]
    pre = g @ w["W1"][:, :E].T + ctab[j][:, None, :]
    h = pre if mutant == "relu_dropped" else torch.relu(pre)
    res = h @ w["W2"].T
    if mutant != "b2_dropped":
        res = res + w["b2"]
    return (res if mutant == "residual_g_dropped" else g + res), pre


def _padded_to_key_tiles(part):
    """`padded_slots_not_zero`: the glimpse runs over 16 ceil(M / 16) slots, the slots beyond M holding the last node's key,
    value and feasibility."""
    M = part["K"].shape[1]
    pad = -M % 16
    out = dict(part)
    for k in ("K", "V", "Lp", "Pa", "Pb"):
        if part.get(k) is not None:
            out[k] = torch.cat([part[k], part[k][:, -1:].expand(-1, pad, -1)], 1)
    out["mask"] = torch.cat([part["mask"], part["mask"][..., -1:].expand(-1, -1, pad)], -1)
    return out


def run(op, dtype=torch.float64, mutant=None, chunk=64, rowwise=False, poly=None):
    """reeval_ref.reeval on `op` in `dtype`, T-chunk by T-chunk (the steps are independent; SDVRP's per-step keys are large),
    plus `logp_all` [R, T, M]: the full log-prob vector of every step, -inf at the infeasible nodes.
    rowwise: u[n] is recomputed from the heads as one sum over the 128 products of node n alone, so that nodes with bit-identical
    rows get bit-identical logits whatever their position -- a property a matrix product of a BLAS does not have at the edge
    columns, and one that `rollout`, standing in for a kernel, needs for its ties.
    poly (or op["poly"]): the PolyNet pointer (module text): u comes from y and op["L"]; the result gains `pre` [R, T, P]."""
    poly = op.get("poly") if poly is None else poly
    assert mutant is None or mutant in MUTANTS or (poly is not None and mutant in POLY_MUTANTS)
    assert poly is None or (op.get("L") is not None and op.get("dyn") is None)
    T = op["actions"].shape[1]
    per_t = ("mask", "idxA", "idxB", "actions", "rem")
    outs = []
    for t0 in range(0, T, chunk):
        part = dict(op)
        for k in per_t:
            if op.get(k) is not None:
                part[k] = op[k][:, t0:t0 + chunk]
        if op.get("sc") is not None:
            part["sc"] = op["sc"][:, :, t0:t0 + chunk]
        part["tstart"] = max(op["tstart"] - t0, 0)
        part = rr.cast(part, dtype)
        glimpse = _padded_to_key_tiles(part) if mutant == "padded_slots_not_zero" and part["K"].shape[1] % 16 else part
        r = rr.reeval(glimpse, mutant if mutant in REEVAL_MUTANTS else None)
        R, nB = part["actions"].shape[0], part["K"].shape[0]
        inst = torch.arange(R) // op["S"] if mutant == "instance_r_div_S" else torch.arange(R) % nB
        if poly is not None:
            y, r["pre"] = polynet_y(r["heads"], poly, nB, mutant)
            Lr = part["Lp" if mutant == "folded_Lp_for_L" else "L"][inst]
            r["u"] = ((y[:, :, None, :] * Lr[:, None]).sum(-1) if rowwise else torch.einsum("rte,rne->rtn", y, Lr)) / math.sqrt(E)
        elif rowwise:
            Lr = part["Lp"][inst][:, None]
            if part.get("dyn") is not None:
                Lr = Lr + part["rem"][..., None] * part["dyn"][2]
            r["u"] = (r["heads"][:, :, None, :] * Lr).sum(-1) / math.sqrt(E)
        r["logp_all"] = logprob_rows(r["u"], part["mask"], op["clip"], op["temp"], mutant)
        if mutant in LOGIT_MUTANTS or rowwise or poly is not None:
            r["logp"] = r["logp_all"].gather(-1, part["actions"][..., None]).squeeze(-1)
        outs.append({k: r[k] for k in ("logp", "lse", "u", "logp_all", "heads") + (("pre",) if poly is not None else ())})
    return {k: torch.cat([o[k] for o in outs], 1) for k in outs[0]}


def logprob_rows(u, mask, clip, temp, mutant=None):
    """The logit processing of utils/decoding.py:140-190 on the raw logits u [R, T, M]: tanh clip, mask, temperature,
    log-softmax."""
    if mutant == "temperature_before_clip":
        z = clip * torch.tanh(u / temp) if clip > 0 else u / temp
        z = z.masked_fill(~mask, -math.inf)
    elif mutant == "mask_before_clip":
        z = u.masked_fill(~mask, -math.inf)
        z = (clip * torch.tanh(z) if clip > 0 else z) / temp
    else:
        z = (clip * torch.tanh(u) if clip > 0 else u).masked_fill(~mask, -math.inf) / temp
    return torch.log_softmax(z, dim=-1)


def keys64(r64, mode, noise=None, mutant=None):
    """The selection key [R, T, M] of a `run` result: the log-probs (greedy), logp - log(noise) (sampling: the reference's
    argmax(p / q), q ~ Exp(1), in the log domain; utils/decoding.py:452-465 draw with the same distribution).  -inf at the
    infeasible nodes."""
    lp = r64["logp_all"]
    if mode == "greedy":
        return lp
    noise = noise.to(lp.dtype)[:, :lp.shape[1]]
    return lp - (noise if mutant == "sampling_minus_noise" else torch.log(noise))


def select(key, mutant=None):
    """argmax over the nodes; the lowest index wins a tie."""
    if mutant == "tie_to_higher_index":
        return key.shape[-1] - 1 - torch.argmax(key.flip(-1), dim=-1)
    return torch.argmax(key, dim=-1)


def rollout(cache, batch, S, mode, noise=None, dtype=torch.float64, clip=10.0, temp=1.0, t_max=None, mutant=None, poly=None):
    """The decode loop on the restatement: every row selects by `keys64` until all rows are done (rows that are done keep
    selecting: their mask allows the depot only) or t_max steps are taken.  -> (actions [R, T] int64, logps [R, T] in `dtype`).
    poly: the PolyNet pointer, where the cache dict does not carry it."""
    env = str(batch["env"])
    states = step_ref.reset_rows(batch, S)
    prev = states
    acts, lps = [], []
    t = 0
    while not all(s["done"] for s in states) and (t_max is None or t < t_max):
        p = step_operands(env, states, prev, mutant if mutant in MUTANTS else None)
        op = _assemble(cache, [p], np.zeros((len(states), 1), np.int64), S, 0, clip, temp)
        r = run(op, dtype, mutant, rowwise=True, poly=poly)
        key = keys64(r, mode, None if noise is None else noise[:, t:t + 1], mutant)[:, 0]
        a = select(key, mutant)
        acts.append(a)
        lps.append(r["logp_all"][:, 0].gather(-1, a[:, None]).squeeze(-1))
        if not all(s["mask"][int(n)] for s, n in zip(states, a)):           # (a mutant's infeasible choice: the rollout ends there)
            break
        prev, states = states, [step_ref.step(s, int(n)) for s, n in zip(states, a)]
        t += 1
    return torch.stack(acts, 1), torch.stack(lps, 1)
