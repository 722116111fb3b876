"""Efficient Active Search (Hottung et al. 2022) with embedding adaptation (EAS-Emb) or layer adaptation (EAS-Lay, last
section) on the native rollout and re-evaluation kernels.  Reference: rl4co/models/zoo/eas/search.py:50-69,137-281 (hyper-parameters, loss, incumbent) and decoder.py:35-126
(the rollout with an incumbent row per instance).

The policy is frozen.  A batch of test instances is augmented and encoded ONCE; the decoder cache of that pass
(ops.DecodeCache) is the search state, and clones of the adapted cache tensors -- by default the logit key alone -- are the
parameters of a torch Adam.  Every iteration

  1. writes the planes derived from the adapted tensors back into the cache (Lp = L Wout by ops.matmul_right),
  2. runs one multistart sampling rollout on that cache (the start-sharing kernel with in-kernel noise, which also keeps every
     step's log-prob and glimpse output),
  3. from iteration 1 on, re-evaluates one incumbent row per augmented instance (the best tour found so far of its original
     instance) by eamrl_reeval_forward on states replayed from its actions,
  4. writes d loss / d logp -- a per-row constant, `eas_loss_coefficients` -- straight into the kernels' upstream gradient, and
  5. takes the gradient: with only the logit key adapted it enters through Lp alone, so two eamrl_reeval_backward_lp launches
     (sampled rows on the rollout's log-probs and heads, incumbent rows on their lse) accumulate one dLp and dL = dLp Wout^T
     (the fast path); any other subset of {logit_key, glimpse_key, glimpse_val}, graphs of 113 .. 1024 nodes and SDVRP go
     through the full backward (train._NativeReeval) with the adapted tensors as autograd leaves (the general path).

Two deviations from the reference, both deliberate: the start nodes are env.select_start_nodes(td, S) as in every
other multistart rollout of this library (the reference's select_start_nodes(td, S + 1) % S maps a depot env's last customer to
the depot), and iteration 0 has no incumbent group and no imitation term (the reference imitates one more sampled row there).

EAS-Lay (use_eas_layer=True, use_eas_embedding=False; zoo/eas/nn.py:5-30, decoder.py:12-32): the cache stays as it is and the
parameters are one residual layer per augmented instance, y = h + relu(h W1 + b1) W2 + b2 on the glimpse output h before
project_out, kept for the whole search in the kernels' layout (ops.pack_eas_layer; Adam is element-wise).  Every iteration is ONE
rollout of S + 1 rows per instance on the layer case of the start-sharing kernel -- from iteration 1 on the last row is forced
to the incumbent, as the reference's row S + 1 (decoder.py:73-79,111-115) -- and ONE eamrl_eas_layer_backward launch over all
rows, on the rollout's own log-probs and captured heads.  TSP and CVRP, at most 112 nodes, S + 1 <= 128.
"""
from __future__ import annotations

import time

import torch

from . import ops
from .utils import StateAugmentation

CACHE_KEYS = {"logit_key": "L", "glimpse_key": "K", "glimpse_val": "V"}      # PrecomputedCache field -> cache slot
BASELINES = ("multistart", "symmetric", "full")
LAYER_ENVS = ("tsp", "cvrp")        # EAS-Lay: the envs of the rollout kernel's layer case
LAYER_PARAMS = ("W1", "b1", "W2", "b2")


def eas_layer_init(N: int, E: int, generator=None):
    """The reference's initialisation of EASLayerNet on the reference's shapes (zoo/eas/nn.py:14-24): W1 [N, E, E] and b1 [N, 1, E]
    by xavier_uniform_ (torch's fan rule for those shapes: fan_in = E * E and N * E for W1, E and N * E for b1), W2 = b2 = 0.
    CPU tensors."""
    W1, b1 = torch.empty(N, E, E), torch.empty(N, 1, E)
    kw = {} if generator is None else {"generator": generator}
    torch.nn.init.xavier_uniform_(W1, **kw)
    torch.nn.init.xavier_uniform_(b1, **kw)
    return W1, b1, torch.zeros(N, E, E), torch.zeros(N, 1, E)


def eas_loss_coefficients(reward, baseline: str, eas_lambda: float, incumbent: bool):
    """d loss / d ll of one EAS iteration, loss = -mean(adv * ll_sampled) + eas_lambda * (-mean(ll_incumbent))
    (zoo/eas/search.py:223-241).  reward [B, n_aug, S]: the rewards of the sampled rows (the incumbent's reward enters neither the
    baseline nor the loss).  -> [B, n_aug, S + 1] with the incumbent's coefficient in the last column, or [B, n_aug, S] without an
    incumbent group.  Plain torch on whatever device and dtype `reward` has."""
    if baseline == "multistart":
        bl = reward.mean(dim=-1, keepdim=True)
    elif baseline == "symmetric":
        bl = reward.mean(dim=-2, keepdim=True)
    elif baseline == "full":
        bl = reward.mean(dim=-1, keepdim=True).mean(dim=-2, keepdim=True)
    else:
        raise ValueError(f"Baseline {baseline} not supported.")
    coef = -(reward - bl) / reward.numel()
    if incumbent:
        inc = torch.full_like(reward[..., :1], -float(eas_lambda) / (reward.shape[0] * reward.shape[1]))
        coef = torch.cat((coef, inc), dim=-1)
    return coef


def eas_layer_row_coefficients(coef):
    """[B, n_aug, G] coefficients (`eas_loss_coefficients`) -> [G * n_aug * B], one per row of the layer rollout: rows in "(s b)"
    order over the augmented batch, row (g * n_aug + a) * B + b, so the forced (incumbent) group g = G - 1 comes last."""
    return coef.permute(2, 1, 0).reshape(-1)


def _pad_to(actions, width: int):
    """Depot visits up to `width` columns (a finished row stays at the depot with probability 1)."""
    if actions.shape[1] >= width:
        return actions
    return torch.cat((actions, actions.new_zeros(actions.shape[0], width - actions.shape[1])), 1)


class _State:
    """What one `search` call keeps between its iterations."""


class EAS:
    """EAS-Emb test-time search.  `search(td)` adapts the cached embeddings of the batch `td` (a reset TensorDict on the GPU)
    for `max_iters` iterations and returns {"max_reward": [B] float32, "best_solutions": [B, T] int64}.  The policy's parameters,
    their requires_grad flags and its buffers are never written.  No Lightning and no dataset plumbing: the caller batches.

    Names and defaults are the reference's (zoo/eas/search.py:50-69).  use_eas_layer=True with use_eas_embedding=False is EAS-Lay
    (module docstring).  The layer has no CPU path: a layer search whose policy parameters are not on a GPU raises
    NotImplementedError at construction, before anything else is looked at.  Also NotImplementedError, each naming its limit:
    both adaptations at once, a layer search on an env other than TSP / CVRP (here), above 112 nodes or with S + 1 > 128 rows
    per instance (in `begin`, where the batch is known), num_parallel_runs != 1 (the reference's incumbent indexing is not well
    defined for it) and an env without native re-evaluation (PDP).
    seed: seeds the rollouts' counter-based noise (None: torch's global generator, as the policy's own sampling rollouts)."""

    def __init__(self, env, policy, use_eas_embedding: bool = True, use_eas_layer: bool = False,
                 eas_emb_cache_keys=("logit_key",), eas_lambda: float = 0.013, max_iters: int = 200, augment_size: int = 8,
                 augment_dihedral: bool = True, num_parallel_runs: int = 1, baseline: str = "multistart",
                 max_runtime: float = 86_400, optimizer_kwargs=None, seed=None):
        from .train import _NATIVE_ENVS

        assert use_eas_embedding or use_eas_layer, "At least one of `use_eas_embedding` or `use_eas_layer` must be True."
        if getattr(policy, "is_ptrnet", False):
            raise NotImplementedError("EAS: the Pointer Network policy has no cached embeddings or pointer layer to adapt; EAS is "
                                      "not built for it")
        if use_eas_layer:
            if not all(p.is_cuda for p in policy.parameters()):
                raise NotImplementedError("EAS-Lay: the per-instance layer runs inside the GPU rollout kernel and has no CPU path; "
                                          "move the policy to the GPU")
            if use_eas_embedding:
                raise NotImplementedError("EAS: use_eas_embedding and use_eas_layer together are not built; choose one")
            if policy.env_name not in LAYER_ENVS:
                raise NotImplementedError(f"EAS-Lay: env {policy.env_name!r} is not built; the layer rollout serves {LAYER_ENVS}")
        self.layer = bool(use_eas_layer)
        if num_parallel_runs != 1:
            raise NotImplementedError("num_parallel_runs != 1: the reference's incumbent indexing is not well defined for it")
        assert baseline in BASELINES, f"Baseline {baseline} not supported."
        keys = list(eas_emb_cache_keys)
        if not keys or any(k not in CACHE_KEYS for k in keys) or len(set(keys)) != len(keys):
            raise ValueError(f"eas_emb_cache_keys must be a non-empty subset of {sorted(CACHE_KEYS)}, got {keys}")
        if policy.env_name not in _NATIVE_ENVS:
            raise NotImplementedError(f"EAS needs the native re-evaluation kernels, which do not cover {policy.env_name!r}")
        self.env, self.policy, self.keys = env, policy, keys
        self.eas_lambda, self.max_iters, self.baseline, self.max_runtime = float(eas_lambda), int(max_iters), baseline, max_runtime
        self.augmentation = StateAugmentation(num_augment=augment_size, augment_fn="dihedral8" if augment_dihedral else "symmetric")
        self.optimizer_kwargs = dict({"lr": 0.0041, "weight_decay": 1e-6} if optimizer_kwargs is None else optimizer_kwargs)
        self.seed = seed
        self.force_general = False          # measurements and tests: the general path where the fast one applies

    # ---- once per batch ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def begin(self, td, seed=None) -> _State:
        """Augment, encode, precompute the cache, clone the adapted tensors and create the optimizer."""
        from .train import native_reeval_supported

        ops._need_gpu(td["locs"], "TensorDict")
        pol, env = self.policy, self.env
        s = _State()
        s.td0 = td
        s.B = td["action_mask"].shape[0]
        s.S = int(env.get_num_starts(td))
        s.td = self.augmentation(td)
        s.n_aug = self.augmentation.num_augment
        s.Ba = s.B * s.n_aug
        s.M = td["action_mask"].shape[-1]
        if not native_reeval_supported(pol, s.M):
            raise NotImplementedError(f"EAS: no native re-evaluation for {pol.env_name!r} with {s.M} nodes")
        was_training = pol.training         # test-time search: batch norm reads its running statistics and never updates them
        pol.eval()
        try:
            hidden, _ = pol.encoder(s.td)
            s.cache = pol.decoder._precompute_cache(hidden)
        finally:
            pol.train(was_training)
        seed = self.seed if seed is None else seed
        s.gen = None if seed is None else torch.Generator().manual_seed(int(seed))
        s.max_reward = torch.full((s.B,), -float("inf"), device=td["locs"].device)
        s.best = None           # [B, W] int64 once an iteration has run
        s.iter = 0
        if self.layer:
            return self._begin_layer(s)
        s.Wout = pol.decoder.pointer.project_out.weight.detach().contiguous()
        s.WoutT = s.Wout.t().contiguous()
        s.params = {k: torch.nn.Parameter(s.cache.view(CACHE_KEYS[k]).clone().contiguous()) for k in self.keys}
        s.opt = torch.optim.Adam(list(s.params.values()), **self.optimizer_kwargs)
        s.fast = (self.keys == ["logit_key"] and s.M <= ops.KEY_CHUNK and s.cache.dyn is None and not s.cache.planes)
        return s

    def _plane(self, s: _State, slot: str):
        """The cache's rows of `slot` as a [B M, E] view (both cache layouts)."""
        c = s.cache
        if c.planes:
            return c.buf[c.slots[slot]].view(c.B * c.M, c.E)
        return c.buf.view(c.B * c.M, -1)[:, c.slots[slot] * c.E:(c.slots[slot] + 1) * c.E]

    @torch.no_grad()
    def _refresh(self, s: _State):
        """The cache planes derived from the adapted tensors, in place (decoder.py:96 reads the adapted cache every step)."""
        for k, p in s.params.items():
            self._plane(s, CACHE_KEYS[k]).copy_(p.detach().view(-1, s.cache.E))
        if "logit_key" in s.params:
            ops.matmul_right(s.params["logit_key"].detach(), s.Wout, out=self._plane(s, "Lp"))

    # ---- one iteration -----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _multistart_rollout(self, s: _State, extra_start=None, **rollout_kw):
        """Multistart sampling rollout on the search's cache: what policy._enqueue does for one, on a given cache.  extra_start
        [Ba]: one more row per instance behind the S multistart rows, starting there; rollout_kw goes to ops.rollout.
        -> actions [R, T] (start column included), logp [R, T], heads [R, >= T - 1, E] or None, reward [R]"""
        from .policy import _env_step_, _max_decode_steps, state_from_td

        pol, env = self.policy, self.env
        st = state_from_td(pol.env_name, s.td, s.S + (0 if extra_start is None else 1))
        start = env.select_start_nodes(s.td, num_starts=s.S).to(torch.int64)
        if extra_start is not None:
            start = torch.cat((start, extra_start))
        start = start.contiguous()
        _env_step_(st, start)
        t_max = int(max(1, _max_decode_steps(pol.env_name, s.M, 1)))
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=s.gen).item())
        acts, lps, info = ops.rollout(st, s.cache, "sampling", clip=pol.tanh_clipping, temp=pol.temperature, t_max=t_max, seed=seed,
                                      want_heads=True, **rollout_kw)
        T, status = info.tolist()
        ops.raise_on_status(status)
        actions = torch.cat((start[:, None], acts[:, :T]), 1).contiguous()
        logp = torch.cat((torch.zeros_like(lps[:, :1]), lps[:, :T]), 1).contiguous()
        reward = env.get_reward(s.td, actions, check_solution=False)
        return actions, logp, st.heads, reward

    def _rollout(self, s: _State):
        """The rollout of an iteration on the adapted cache."""
        return self._multistart_rollout(s)

    def _plan(self, s: _State, actions, S: int, rollout_logp=None, rollout_heads=None):
        """A re-evaluation plan that reads the adapted cache in place."""
        from .train import replay_states

        pol, c = self.policy, s.cache
        meta = replay_states(pol, s.td, actions, S, True)
        if pol.env_name == "tsp":
            cvec = None                     # (multistart: no placeholder step)
        else:
            cvec = c.cvec.reshape(-1, c.E).contiguous()
        slots = {n: c.slots[n] for n in ("K", "V", "Lp", "Pa") + (("Pb",) if "Pb" in c.slots else ())}
        return ops.ReevalPlan(c.buf, "Pb" in c.slots, c.gctx, cvec, meta["idxA"], meta["idxB"], meta["sc"], meta["maskbits"],
                              actions, S, meta["tstart"], float(pol.tanh_clipping), float(pol.temperature), slots=slots, E=c.E,
                              rollout_logp=rollout_logp, rollout_heads=rollout_heads)

    def _rows(self, s: _State, coef):
        """[B, n_aug, G] coefficients -> per-row vectors in the rollout's (s a b) row order: sampled rows, incumbent rows or None."""
        sampled = coef[..., :s.S].permute(2, 1, 0).reshape(-1)
        inc = coef[..., s.S].permute(1, 0).reshape(-1) if coef.shape[-1] > s.S else None
        return sampled, inc

    def _decoder_tensors(self, s: _State):
        """train.decoder_tensors of the frozen policy with the adapted tensors in place of their cache rows (general path)."""
        pol, c = self.policy, s.cache
        dec = pol.decoder
        t = {"emb": c.node_embeddings, "Wctx": dec.context_embedding.project_context.weight.detach(), "Wout": s.Wout}
        for k, slot in CACHE_KEYS.items():
            t[slot] = s.params[k] if k in s.params else c.view(slot).contiguous()
        if dec.use_graph_context:
            t["gctx"] = c.gctx
        if pol.env_name == "tsp":
            t["placeholder"] = dec.context_embedding.W_placeholder.detach()
        if pol.env_name == "sdvrp":
            t["dyn"] = dec.dynamic_embedding.projection.weight.detach()
        return t

    # ---- EAS-Lay -----------------------------------------------------------------------------------------------------
    def _begin_layer(self, s: _State) -> _State:
        """The layer's parameters (one set per augmented instance, kernel layout) and their Adam."""
        pol, c = self.policy, s.cache
        if s.M > ops.KEY_CHUNK or c.planes:
            raise NotImplementedError(f"EAS-Lay: graphs above {ops.KEY_CHUNK} nodes are not built ({s.M} nodes)")
        if s.S + 1 > 128:
            raise NotImplementedError(f"EAS-Lay: S + 1 = {s.S + 1} rows per instance; the layer rollout takes at most 128")
        if not ops.rollout_eas_layer_supported(pol.env_name, c, (s.S + 1) * s.Ba):
            raise NotImplementedError("EAS-Lay: this decoder shape is not built (embed_dim 128, 8 heads, 2 .. 112 nodes)")
        dev = s.td["locs"].device
        W1, b1, W2, b2 = eas_layer_init(s.Ba, c.E, s.gen)
        s.params = {"W1": torch.nn.Parameter(ops.pack_eas_layer(W1).to(dev)), "b1": torch.nn.Parameter(b1.reshape(s.Ba, c.E).to(dev)),
                    "W2": torch.nn.Parameter(ops.pack_eas_layer(W2).to(dev)), "b2": torch.nn.Parameter(b2.reshape(s.Ba, c.E).to(dev))}
        s.opt = torch.optim.Adam(list(s.params.values()), **self.optimizer_kwargs)
        s.fast = False
        return s

    def _layer_operands(self, s: _State, forced=None):
        d = {n: s.params[n].detach() for n in LAYER_PARAMS}
        if forced is not None:
            d["forced"] = forced
        return d

    def _rollout_layer(self, s: _State):
        """One sampling rollout of S (+ 1 with an incumbent) rows per instance through the layer; the last row follows the incumbent.
        -> `_multistart_rollout`'s tuple (heads: pre-layer) and the rows per instance"""
        if s.best is None:
            return self._multistart_rollout(s, eas_layer=self._layer_operands(s)) + (s.S,)
        tour = s.best.repeat(s.n_aug, 1)                            # rows (a b) <- best[b]
        forced = tour[:, 1:].contiguous()
        return self._multistart_rollout(s, tour[:, 0], eas_layer=self._layer_operands(s, forced)) + (s.S + 1,)

    def _iteration_layer(self, s: _State, rollout=None) -> dict:
        actions, logp, heads, reward, S1 = rollout if rollout is not None else self._rollout_layer(s)
        R, T = actions.shape
        ns = s.S * s.Ba                                             # the sampled rows come first ((s b) order, incumbent group last)
        inc = S1 > s.S
        r3 = reward[:ns].view(s.S, s.n_aug, s.B).permute(2, 1, 0)   # [B, n_aug, S]
        coef = eas_loss_coefficients(r3, self.baseline, self.eas_lambda, incumbent=inc)
        g = eas_layer_row_coefficients(coef)[:, None].expand(R, T).contiguous()
        with torch.no_grad():
            grads = self._plan(s, actions, S1, rollout_logp=logp, rollout_heads=heads).backward_layer(g, self._layer_operands(s))
        for n in LAYER_PARAMS:
            s.params[n].grad = grads[n]
        return dict(actions=actions[:ns], reward=reward[:ns], logp=logp[:ns], rollout=(actions, logp, heads, reward, S1),
                    inc_actions=actions[ns:] if inc else None, inc_reward=reward[ns:] if inc else None, coef=coef, grads=grads)

    def iteration(self, s: _State, general=None, rollout=None) -> dict:
        """Refresh, rollout, incumbent rows and the gradient of the adapted tensors (left in their .grad); no optimizer step.
        general: force the general (True) or the fast (False) backward; rollout: the `rollout` entry of an earlier call on the same
        state, taken instead of a new rollout (the two paths on the same tours).
        -> dict(actions, reward, logp, rollout, inc_actions, inc_reward, coef, grads)"""
        if self.layer:
            return self._iteration_layer(s, rollout)
        pol, env = self.policy, self.env
        general = (not s.fast or self.force_general) if general is None else general
        if not general and not s.fast:
            raise ValueError("EAS: the fast path needs keys == ['logit_key'], at most 112 nodes and no dynamic embedding")
        self._refresh(s)
        actions, logp, heads, reward = rollout if rollout is not None else self._rollout(s)
        R, T = actions.shape
        inc = inc_reward = None
        if s.best is not None:              # one incumbent row per augmented instance: rows (a b) <- best[b]
            with torch.no_grad():
                inc = s.best.repeat(s.n_aug, 1).contiguous()
                inc_reward = env.get_reward(s.td, inc, check_solution=False)
        r3 = reward.view(s.S, s.n_aug, s.B).permute(2, 1, 0)                       # [B, n_aug, S]
        coef = eas_loss_coefficients(r3, self.baseline, self.eas_lambda, incumbent=inc is not None)
        cs, ci = self._rows(s, coef)
        g_s = cs[:, None].expand(R, T).contiguous()
        g_i = ci[:, None].expand(*inc.shape).contiguous() if inc is not None else None
        for p in s.params.values():
            p.grad = None
        if not general:
            with torch.no_grad():
                dLp = self._plan(s, actions, s.S, rollout_logp=logp, rollout_heads=heads).backward_lp(g_s)
                if inc is not None:
                    plan = self._plan(s, inc, 1)
                    plan.forward()
                    plan.backward_lp(g_i, out=dLp)
                s.params["logit_key"].grad = ops.matmul_right(dLp, s.WoutT)
        else:
            from .train import _evaluate_native

            t = self._decoder_tensors(s)
            with torch.enable_grad():
                lp = _evaluate_native(pol, t, s.td, actions, s.S, True, pol.temperature, pol.tanh_clipping,
                                      rollout_logp=logp, rollout_heads=heads)
                obj = (g_s * lp).sum()
                if inc is not None:
                    obj = obj + (g_i * _evaluate_native(pol, t, s.td, inc, 1, True, pol.temperature, pol.tanh_clipping)).sum()
            grads = torch.autograd.grad(obj, list(s.params.values()))
            for p, g in zip(s.params.values(), grads):
                p.grad = g
        return dict(actions=actions, reward=reward, logp=logp, rollout=(actions, logp, heads, reward), inc_actions=inc, inc_reward=inc_reward, coef=coef,
                    grads={k: p.grad for k, p in s.params.items()})

    @torch.no_grad()
    def _update_incumbent(self, s: _State, it: dict):
        """The best sampled row of each original instance over its n_aug * S rows replaces the stored tour where it is better.
        (The incumbent rows are the stored tour itself.)  Rewards are compared on the ORIGINAL instance, so that max_reward is
        env.get_reward(td, best_solutions) whichever augmented copy found the tour."""
        actions, reward = it["actions"], it["reward"]
        top = reward.view(s.S, s.n_aug, s.B).permute(2, 1, 0).reshape(s.B, -1).argmax(1)      # index a * S + s_
        a, s_ = top // s.S, top % s.S
        rows = (s_ * s.n_aug + a) * s.B + torch.arange(s.B, device=top.device)
        width = max(actions.shape[1], 0 if s.best is None else s.best.shape[1])
        cand = _pad_to(actions[rows], width).contiguous()
        r = self.env.get_reward(s.td0, cand)
        better = r > s.max_reward
        if s.best is None:
            s.best = cand
        else:
            s.best = torch.where(better[:, None], cand, _pad_to(s.best, width)).contiguous()
        s.max_reward = torch.where(better, r, s.max_reward)

    def step(self, s: _State, general=None) -> dict:
        """One whole EAS iteration: gradient, Adam step, incumbent update."""
        it = self.iteration(s, general)
        s.opt.step()
        self._update_incumbent(s, it)
        s.iter += 1
        return it

    def search(self, td, max_iters=None, seed=None) -> dict:
        s = self.begin(td, seed=seed)
        t_start = time.time()
        for _ in range(self.max_iters if max_iters is None else int(max_iters)):
            self.step(s)
            if time.time() - t_start > self.max_runtime:        # checked on the host, once per iteration
                break
        return {"max_reward": s.max_reward, "best_solutions": s.best}


class EASEmb(EAS):
    """EAS with embedding adaptation (zoo/eas/search.py:311-327)."""

    def __init__(self, *args, **kwargs):
        kwargs["use_eas_embedding"] = True
        kwargs["use_eas_layer"] = False
        super().__init__(*args, **kwargs)


class EASLay(EAS):
    """EAS with layer adaptation (zoo/eas/search.py:330-346): `search(td)` as EASEmb, on one residual layer per augmented
    instance instead of the embeddings.  Needs the policy on a GPU (NotImplementedError otherwise)."""

    def __init__(self, *args, **kwargs):
        kwargs["use_eas_embedding"] = False
        kwargs["use_eas_layer"] = True
        super().__init__(*args, **kwargs)
