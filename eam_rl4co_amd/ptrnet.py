"""Pointer Network policy (Vinyals et al. 2015, Bello et al. 2016; rl4co/models/zoo/ptrnet/{policy,encoder,decoder}.py) for TSP.

Rollouts run natively: `ops.ptrnet_encode` (the encoder LSTM over the nodes, one launch), two `ops.linear` calls (the ref
projections of the glimpse and of the pointer on the encoder's outputs) and `ops.ptrnet_rollout` (the whole decode loop, one
launch) -- no host synchronisation, no per-step launch, no PyTorch rollout off the GPU.  Under autograd (phase="train") the
log-likelihood of the tours the native rollout chose comes from `PointerNetworkPolicy.torch_rollout`, the same model written
with torch ops on the policy's own parameters and teacher-forced on those tours (the PolyNet pattern: there is no native
backward)."""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .envs import RL4COEnvBase


class Encoder(nn.Module):
    """zoo/ptrnet/encoder.py: nn.LSTM(embed_dim, hidden_dim) over the node sequence.  init_hx / init_cx exist in the reference's
    state dict but it never reads them (policy.py:91-96 starts from zeros); they are kept, and unused, here as well."""

    def __init__(self, input_dim, hidden_dim):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.lstm = nn.LSTM(input_dim, hidden_dim)
        std = 1.0 / math.sqrt(hidden_dim)
        self.init_hx = nn.Parameter(torch.empty(hidden_dim).uniform_(-std, std))
        self.init_cx = nn.Parameter(torch.empty(hidden_dim).uniform_(-std, std))


class SimpleAttention(nn.Module):
    """zoo/ptrnet/decoder.py:11-47: u_n = v . tanh(project_query(h) + project_ref(ctx)_n), C tanh(u) if use_tanh."""

    def __init__(self, dim, use_tanh=False, C=10):
        super().__init__()
        self.use_tanh = use_tanh
        self.project_query = nn.Linear(dim, dim)
        self.project_ref = nn.Conv1d(dim, dim, 1, 1)
        self.C = C
        std = 1.0 / math.sqrt(dim)
        self.v = nn.Parameter(torch.empty(dim).uniform_(-std, std))


class Decoder(nn.Module):
    """zoo/ptrnet/decoder.py:50-73 (parameters only: the step loop is the native rollout)."""

    def __init__(self, embed_dim=128, hidden_dim=128, tanh_exploration=10.0, use_tanh=True):
        super().__init__()
        self.lstm = nn.LSTMCell(embed_dim, hidden_dim)
        self.pointer = SimpleAttention(hidden_dim, use_tanh=use_tanh, C=tanh_exploration)
        self.glimpse = SimpleAttention(hidden_dim, use_tanh=False)


def _lstm_cell(x_gates, h, c, w_hh, b_hh):
    gates = x_gates + F.linear(h, w_hh, b_hh)
    i, f, g, o = gates.chunk(4, dim=1)                       # torch's gate order
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


class PointerNetworkPolicy(nn.Module):
    """`PointerNetworkPolicy(env_name="tsp", embed_dim=128, hidden_dim=128, tanh_clipping=10.0, mask_inner=True,
    mask_logits=True)`: the reference's arguments, defaults, parameter names and shapes (so `load_reference_checkpoint` takes a
    Pointer Network checkpoint).  Built: TSP, embed_dim = hidden_dim = 128, 2..128 nodes, one tour per instance, greedy /
    sampling / evaluation of given tours.  Everything else raises NotImplementedError naming its limit."""

    MAX_NODES = ops.PTRNET_MAX_NODES
    is_ptrnet = True         # GraphedRollout, EAS*, PPOStep and eam_am_loss decline this policy by it

    def __init__(self, env_name="tsp", embed_dim: int = 128, hidden_dim: int = 128, tanh_clipping: float = 10.0,
                 mask_inner: bool = True, mask_logits: bool = True, **kwargs):
        super().__init__()
        if isinstance(env_name, RL4COEnvBase):
            env_name = env_name.name
        if env_name != "tsp":
            raise NotImplementedError(f"PointerNetworkPolicy: only the Euclidean TSP env is built (as in the reference), got "
                                      f"env_name={env_name!r}")
        if embed_dim != 128 or hidden_dim != 128:
            raise NotImplementedError(f"PointerNetworkPolicy: the kernels are built for embed_dim = hidden_dim = 128, got "
                                      f"{embed_dim} / {hidden_dim}")
        if not tanh_clipping > 0:
            raise NotImplementedError("PointerNetworkPolicy: tanh_clipping <= 0 (pointer logits without the tanh clip) is not "
                                      "built")
        if not mask_inner or not mask_logits:
            raise NotImplementedError("PointerNetworkPolicy: mask_inner=False / mask_logits=False are not built (the rollout "
                                      "kernel masks visited nodes in the glimpse and in the pointer)")
        self.env_name = env_name
        self.input_dim = 2
        self.tanh_clipping = float(tanh_clipping)
        self.encoder = Encoder(embed_dim, hidden_dim)
        self.decoder = Decoder(embed_dim, hidden_dim, tanh_exploration=tanh_clipping, use_tanh=True)
        std = 1.0 / math.sqrt(embed_dim)
        self.decoder_in_0 = nn.Parameter(torch.empty(embed_dim).uniform_(-std, std))
        self.embedding = nn.Parameter(torch.empty(self.input_dim, embed_dim).uniform_(-std, std))

    # ------------------------------------------------------------------------------------------------------------------
    def _check_call(self, td, env, decode_type, kw):
        name = env.name if isinstance(env, RL4COEnvBase) else (env if isinstance(env, str) else self.env_name)
        if name != "tsp":
            raise NotImplementedError(f"PointerNetworkPolicy: only the TSP env is built, got {name!r}")
        S = kw.get("num_starts") if kw.get("num_starts") is not None else kw.get("num_samples")
        if (S is not None and S > 1) or kw.get("multistart") or kw.get("multisample") or "multistart" in str(decode_type):
            raise NotImplementedError("PointerNetworkPolicy: num_starts > 1 / multistart decode types are not built (the "
                                      "Pointer Network decodes one tour per instance)")
        if "beam_search" in str(decode_type) or kw.get("beam_width"):
            raise NotImplementedError("PointerNetworkPolicy: beam search is not built")
        if kw.get("top_k") or 0.0 < float(kw.get("top_p") or 0.0) < 1.0:
            raise NotImplementedError("PointerNetworkPolicy: top-k / top-p filtering is not built into the rollout kernel")
        if kw.get("return_entropy"):
            raise NotImplementedError("PointerNetworkPolicy: return_entropy is not built (the rollout keeps the chosen node's "
                                      "log-probability only)")
        if decode_type not in ("greedy", "sampling", "evaluate"):
            raise NotImplementedError(f"PointerNetworkPolicy: decode_type={decode_type!r} is not built (greedy, sampling, or "
                                      "actions= / eval_tours=)")
        N = td["locs"].shape[-2]
        if not 2 <= N <= self.MAX_NODES:
            raise NotImplementedError(f"PointerNetworkPolicy: graphs of 2..{self.MAX_NODES} nodes are built, got {N}")

    def native_weights(self):
        """state-dict key -> contiguous fp32 tensor, as the kernels take them (no copies for a float32 policy)."""
        sd = dict(self.named_parameters())
        return {key: sd[key].detach().contiguous() for key, _ in ops.PTRNET_WEIGHTS.values()}

    def _ref_projection(self, att: SimpleAttention, ctx):
        W = att.project_ref.weight.detach().squeeze(-1)
        return ops.linear(ctx, W if W.is_contiguous() else W.contiguous(), att.project_ref.bias.detach())

    def forward(self, td, env=None, phase: str = "train", decode_type: str = "sampling", eval_tours=None, actions=None,
                noise=None, seed=None, return_sum_log_likelihood: bool = True, calc_reward: bool = True, **kw):
        given = actions if actions is not None else eval_tours
        if given is not None:
            decode_type = "evaluate"
        self._check_call(td, env, decode_type, kw)
        if phase == "train":
            self.train()
        else:
            self.eval()
        locs = td["locs"]
        ops._need_gpu(locs, "td['locs']")
        locs = locs.detach().float().contiguous()
        B, N, _ = locs.shape
        if decode_type == "sampling" and noise is None and seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())      # torch's CPU generator: no device round trip
        with torch.no_grad():
            w = self.native_weights()
            ctx, h, c, ws = ops.ptrnet_encode(locs, w)
            e_g = self._ref_projection(self.decoder.glimpse, ctx)
            e_p = self._ref_projection(self.decoder.pointer, ctx)
            acts, logp = ops.ptrnet_rollout(
                locs, w, h, c, e_g, e_p, clip=self.tanh_clipping, mode=decode_type,
                noise=None if noise is None else noise.detach().float().contiguous(),
                given=None if given is None else given.detach().long().contiguous(), seed=seed, ws=ws)
            reward = ops.tour_length_reward(locs, acts, False) if calc_reward else None
        if phase == "train" and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            logp = self.torch_rollout(locs, "evaluate", given=acts)[1]
        out = {"reward": reward, "log_likelihood": logp.sum(1) if return_sum_log_likelihood else logp, "actions": acts}
        return out

    # ------------------------------------------------------------------------------------------------------------------
    def torch_rollout(self, locs, mode="greedy", given=None, noise=None):
        """The same model with torch ops on the policy's parameters (differentiable): -> actions [B, N], logp [B, N].  This is the
        training path's teacher-forced expression (mode="evaluate", given=the native tours) and the PyTorch baseline that
        tools/time_ptrnet.py times; it is never a fallback of `forward`."""
        B, N, _ = locs.shape
        enc, dec = self.encoder.lstm, self.decoder
        x = locs @ self.embedding                                              # [B, N, E]
        h = c = locs.new_zeros(B, self.encoder.hidden_dim)
        xg = F.linear(x, enc.weight_ih_l0, enc.bias_ih_l0)
        ctx = []
        for n in range(N):
            h, c = _lstm_cell(xg[:, n], h, c, enc.weight_hh_l0, enc.bias_hh_l0)
            ctx.append(h)
        ctx = torch.stack(ctx, 1)                                              # [B, N, H]
        e_g = F.linear(ctx, dec.glimpse.project_ref.weight.squeeze(-1), dec.glimpse.project_ref.bias)
        e_p = F.linear(ctx, dec.pointer.project_ref.weight.squeeze(-1), dec.pointer.project_ref.bias)
        dg = F.linear(x, dec.lstm.weight_ih, dec.lstm.bias_ih)                 # decoder input gates of every node
        din = F.linear(self.decoder_in_0, dec.lstm.weight_ih, dec.lstm.bias_ih).expand(B, -1)
        visited = torch.zeros(B, N, dtype=torch.bool, device=locs.device)
        acts, lps = [], []
        for t in range(N):
            h, c = _lstm_cell(din, h, c, dec.lstm.weight_hh, dec.lstm.bias_hh)
            u = (torch.tanh(dec.glimpse.project_query(h)[:, None, :] + e_g) * dec.glimpse.v).sum(-1)
            p = torch.softmax(u.masked_fill(visited, float("-inf")), dim=1)
            g = (p[:, :, None] * e_g).sum(1)
            u = (torch.tanh(dec.pointer.project_query(g)[:, None, :] + e_p) * dec.pointer.v).sum(-1)
            logits = (self.tanh_clipping * torch.tanh(u)).masked_fill(visited, float("-inf"))
            lp = torch.log_softmax(logits, dim=1)
            if mode == "evaluate":
                sel = given[:, t]
            elif mode == "sampling":
                sel = (lp.detach().exp() / noise[:, t]).masked_fill(visited, float("-inf")).argmax(1)
            else:
                sel = lp.detach().argmax(1)
            acts.append(sel)
            lps.append(lp.gather(1, sel[:, None]).squeeze(1))
            visited = visited.scatter(1, sel[:, None], True)
            din = dg.gather(1, sel[:, None, None].expand(B, 1, dg.shape[-1])).squeeze(1)
        return torch.stack(acts, 1), torch.stack(lps, 1)
