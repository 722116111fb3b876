"""AttentionModelPolicy on MI355X kernels, behind the reference's module tree and forward signature.

Reference interfaces mirrored (same constructor arguments, state_dict keys, forward kwargs, output dict):
  rl4co/models/zoo/am/policy.py:10-122             AttentionModelPolicy
  rl4co/models/zoo/am/encoder.py:14-91             AttentionModelEncoder
  rl4co/models/zoo/am/decoder.py:22-235            AttentionModelDecoder / PrecomputedCache
  rl4co/models/common/constructive/base.py:157-275 ConstructivePolicy.forward (the rollout)
  rl4co/utils/decoding.py:17-35,193-465            decode-type registry, multistart hooks
The nn.Module tree only exists to hold parameters under the reference's names (checkpoint contract,
tests/golden/state_dict_contract.json); every forward computation is a libeamrl_hip.so launch.
No CPU / PyTorch implementation of the rollout exists here: tensors must live on the GPU.
"""
from __future__ import annotations

import logging
import os
from typing import Optional

import torch
import torch.nn as nn

from . import ops
from .env_spec import ACTION, ALIASES, ENV_SPECS, max_steps
from .envs import ENV_REGISTRY, RL4COEnvBase, get_env
from .tensordict_lite import TensorDict  # noqa: F401
from .utils import unbatchify, unbatchify_and_gather

log = logging.getLogger(__name__)

DECODE_TYPES = ("greedy", "sampling", "multistart_greedy", "multistart_sampling", "evaluate")

# AttentionModelPolicy(precision=...): Lightning's names -> the operand type of the fused encoder (None = fp32)
PRECISIONS = {"32-true": None, "16-mixed": torch.float16, "bf16-mixed": torch.bfloat16}


def _kind(env_name):
    if isinstance(env_name, RL4COEnvBase):
        env_name = env_name.name
    return ALIASES.get(env_name, env_name)


# ------------------------------------------------------------------------------------------------------------
# parameter containers (names = reference state_dict keys)
# ------------------------------------------------------------------------------------------------------------
class TSPInitEmbedding(nn.Module):
    def __init__(self, embed_dim, linear_bias=True):
        super().__init__()
        self.init_embed = nn.Linear(2, embed_dim, linear_bias)

    def forward(self, td):
        return ops.linear(td["locs"].contiguous(), self.init_embed.weight, self.init_embed.bias)

    def fused_spec(self, td):
        """struct eamrl_encoder_init: the fused encoder kernel computes this Linear itself (ops.encoder_fused(init=...))."""
        return dict(feat=td["locs"].contiguous(), W=self.init_embed.weight.detach(),
                    b=None if self.init_embed.bias is None else self.init_embed.bias.detach())


def _depot_fused_spec(mod, locs, feat):
    """struct eamrl_encoder_init of a depot env: customer features zero-padded to one row per node (row 0 unused), the depot
    row from the coordinates (`_depot_and_customers` inside the fused kernel)."""
    if feat.shape[-1] > 8 or mod.init_embed_depot.weight.shape[1] != 2:
        return None
    locs = locs.contiguous()
    bias = lambda lin: None if lin.bias is None else lin.bias.detach()
    return dict(feat=torch.nn.functional.pad(feat, (0, 0, 1, 0)).contiguous(), W=mod.init_embed.weight.detach().contiguous(),
                b=bias(mod.init_embed), depot=locs[:, 0, :], Wd=mod.init_embed_depot.weight.detach().contiguous(),
                bd=bias(mod.init_embed_depot))


def _depot_and_customers(mod, locs, feat):
    """[B, M, E] init embeddings of a depot env: row 0 = init_embed_depot(depot), rows 1.. = init_embed(customer features).
    Both linears write straight into the result (no concatenation of [B, M, E] tensors): the customer linear runs over
    all B*M rows of the zero-padded feature tensor -- one uniform row stride -- and the depot linear then overwrites
    row 0 of every instance.  Same values as the two separate linears."""
    B, M, _ = locs.shape
    E = mod.init_embed.weight.shape[0]
    out = torch.empty(B, M, E, device=locs.device, dtype=torch.float32)
    if B * M == 0:
        return out
    feat_all = torch.nn.functional.pad(feat, (0, 0, 1, 0))                   # [B, M, F], row 0 unused
    ops.linear(feat_all, mod.init_embed.weight, mod.init_embed.bias, out=out)
    ops.linear(locs[:, 0, :], mod.init_embed_depot.weight, mod.init_embed_depot.bias, out=out[:, 0, :])
    return out


class VRPInitEmbedding(nn.Module):
    def __init__(self, embed_dim, linear_bias=True, node_dim: int = 3):
        super().__init__()
        self.init_embed = nn.Linear(node_dim, embed_dim, linear_bias)
        self.init_embed_depot = nn.Linear(2, embed_dim, linear_bias)

    def forward(self, td):
        locs = td["locs"]
        feat = torch.cat((locs[:, 1:, :], td["demand"][..., None]), -1)   # [B, N, 3] input assembly (plumbing)
        return _depot_and_customers(self, locs, feat)

    def fused_spec(self, td):
        locs = td["locs"]
        return _depot_fused_spec(self, locs, torch.cat((locs[:, 1:, :], td["demand"][..., None]), -1))


class PCTSPInitEmbedding(nn.Module):
    """x, y, expected prize, penalty per customer; depot embedded separately (nn/env_embeddings/init.py:227-257)."""

    def __init__(self, embed_dim, linear_bias=True):
        super().__init__()
        self.init_embed = nn.Linear(4, embed_dim, linear_bias)
        self.init_embed_depot = nn.Linear(2, embed_dim, linear_bias)

    def forward(self, td):
        locs = td["locs"]
        feat = torch.cat((locs[:, 1:, :], td["expected_prize"][..., None], td["penalty"][..., 1:, None]), -1)
        return _depot_and_customers(self, locs, feat)

    def fused_spec(self, td):
        locs = td["locs"]
        return _depot_fused_spec(self, locs, torch.cat((locs[:, 1:, :], td["expected_prize"][..., None],
                                                        td["penalty"][..., 1:, None]), -1))


class VRPTWInitEmbedding(nn.Module):
    """x, y, demand, window start, window end, service time per customer (nn/env_embeddings/init.py:141-157)."""

    def __init__(self, embed_dim, linear_bias=True):
        super().__init__()
        self.init_embed = nn.Linear(6, embed_dim, linear_bias)
        self.init_embed_depot = nn.Linear(2, embed_dim, linear_bias)

    def forward(self, td):
        locs = td["locs"]
        depot = ops.linear(locs[:, :1, :].contiguous(), self.init_embed_depot.weight, self.init_embed_depot.bias)
        feat = torch.cat((locs[:, 1:, :], td["demand"][..., None], td["time_windows"][..., 1:, :].to(torch.float32),
                          td["durations"][..., 1:, None]), -1)
        cust = ops.linear(feat, self.init_embed.weight, self.init_embed.bias)
        return torch.cat((depot, cust), 1)

    def fused_spec(self, td):
        locs = td["locs"]
        return _depot_fused_spec(self, locs, torch.cat((locs[:, 1:, :], td["demand"][..., None],
                                                        td["time_windows"][..., 1:, :].to(torch.float32),
                                                        td["durations"][..., 1:, None]), -1))


class OPInitEmbedding(nn.Module):
    """x, y, prize per customer; depot embedded separately (nn/env_embeddings/init.py:260-286)."""

    def __init__(self, embed_dim, linear_bias=True):
        super().__init__()
        self.init_embed = nn.Linear(3, embed_dim, linear_bias)
        self.init_embed_depot = nn.Linear(2, embed_dim, linear_bias)

    def forward(self, td):
        locs = td["locs"]
        feat = torch.cat((locs[:, 1:, :], td["prize"][..., 1:, None]), -1)
        return _depot_and_customers(self, locs, feat)

    def fused_spec(self, td):
        locs = td["locs"]
        return _depot_fused_spec(self, locs, torch.cat((locs[:, 1:, :], td["prize"][..., 1:, None]), -1))


class PDPInitEmbedding(nn.Module):
    """Depot, pickups (with their delivery's coordinates) and deliveries embedded by three Linears
    (nn/env_embeddings/init.py:347-372); one launch (eamrl_pdp_init_embedding), bit-identical to the three `ops.linear` calls.
    The result feeds the fused encoder through its h_in entry (no `fused_spec`: the in-kernel init embedding is one Linear
    plus a depot row)."""

    def __init__(self, embed_dim, linear_bias=True):
        super().__init__()
        self.init_embed_depot = nn.Linear(2, embed_dim, linear_bias)
        self.init_embed_pick = nn.Linear(4, embed_dim, linear_bias)
        self.init_embed_delivery = nn.Linear(2, embed_dim, linear_bias)

    def forward(self, td):
        d, p, l = self.init_embed_depot, self.init_embed_pick, self.init_embed_delivery
        det = lambda t: None if t is None else t.detach().contiguous()
        return ops.pdp_init_embedding(td["locs"].contiguous(), det(d.weight), det(d.bias), det(p.weight), det(p.bias),
                                      det(l.weight), det(l.bias))


class _Holder(nn.Module):
    """`.module` wrapper so that parameter names match the reference's SkipConnection(...)."""

    def __init__(self, module):
        super().__init__()
        self.module = module


class _MHAParams(nn.Module):
    def __init__(self, embed_dim, num_heads, bias=True):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.Wqkv = nn.Linear(embed_dim, 3 * embed_dim, bias=bias)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)


class _MLPParams(nn.Module):
    def __init__(self, input_dim, output_dim, num_neurons):
        super().__init__()
        dims = [input_dim] + list(num_neurons) + [output_dim]
        self.lins = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))


class MoE(nn.Module):
    """Parameters of the reference's sparsely gated mixture of experts (nn/moe.py:114-146, its names and its initialisation:
    `w_gate` = `w_noise` = 0, default Linear experts, buffers `mean` / `std`) as the feed-forward sublayer of an encoder layer
    (MVMoE, Zhou et al. 2024).  `sublayer` is the native forward (ops.moe_ffn: gate, grouped expert GEMM, combine); under
    autograd the gate is a torch expression and the experts run on `train._MoEExpertsFn` (native sparse forward and backward;
    `train.moe_autograd`, the all-torch expression, off the GPU or with EAMRL_MOE_NATIVE_BACKWARD=0).  Extra keyword arguments
    (e.g. `routing_level`) are swallowed, as the reference's constructor does."""

    def __init__(self, input_size, output_size, num_neurons=(), hidden_act="ReLU", out_bias=True, num_experts=4, k=2,
                 noisy_gating=True, **kwargs):
        super().__init__()
        num_neurons = list(num_neurons)
        if input_size != ops.MOE_EMBED_DIM or output_size != ops.MOE_EMBED_DIM or num_neurons != [ops.MOE_HIDDEN]:
            raise NotImplementedError(f"MoE encoder: embed_dim {input_size} -> {num_neurons} -> {output_size}; the expert kernel is "
                                      f"built for embed_dim {ops.MOE_EMBED_DIM} and feedforward_hidden {ops.MOE_HIDDEN}")
        if hidden_act != "ReLU":
            raise NotImplementedError(f"MoE encoder: hidden_act={hidden_act!r}; the expert kernel is built for 'ReLU'")
        if not (isinstance(num_experts, int) and isinstance(k, int) and 1 <= k <= num_experts <= ops.MOE_MAX_EXPERTS):
            raise NotImplementedError(f"MoE encoder: k={k}, num_experts={num_experts}; built for 1 <= k <= num_experts <= "
                                      f"{ops.MOE_MAX_EXPERTS}")
        self.noisy_gating, self.num_experts, self.k = bool(noisy_gating), num_experts, k
        self.input_size, self.output_size = input_size, output_size
        self.experts = nn.ModuleList(_MLPParams(input_size, output_size, num_neurons) for _ in range(num_experts))
        self.w_gate = nn.Parameter(torch.zeros(input_size, num_experts), requires_grad=True)
        self.w_noise = nn.Parameter(torch.zeros(input_size, num_experts), requires_grad=True)
        self.register_buffer("mean", torch.tensor([0.0]))
        self.register_buffer("std", torch.tensor([1.0]))

    def packed_experts(self):
        """The operand dict of ops.moe_ffn: the experts' weights in fragment order and their biases, in persistent buffers
        refreshed in place when a parameter changes (a captured HIP graph keeps reading them), as `_fused_layers` keeps its packs."""
        ps = [p for ex in self.experts for lin in ex.lins for p in (lin.weight, lin.bias)]
        key = tuple((p.data_ptr(), p._version) for p in ps) + (ps[0].device,)
        slot = self.__dict__.get("_packed")
        if slot is None or slot[0] != key:
            buf = None if slot is None or slot[1]["W1p"].device != ps[0].device else slot[1]
            with torch.no_grad():
                buf = ops.pack_moe_experts([ex.lins[0].weight.detach() for ex in self.experts],
                                           [ex.lins[0].bias.detach() for ex in self.experts],
                                           [ex.lins[1].weight.detach() for ex in self.experts],
                                           [ex.lins[1].bias.detach() for ex in self.experts], out=buf)
            self.__dict__["_packed"] = slot = (key, buf)
        return slot[1]

    def packed_experts_backward(self):
        """`packed_experts()` plus the transposed packs the experts' native backward reads (ops.pack_moe_experts_backward), kept
        and refreshed by parameter version in the same way: the operand dict of train._MoEExpertsFn."""
        fwd = self.packed_experts()
        key = self.__dict__["_packed"][0]
        slot = self.__dict__.get("_packed_bwd")
        if slot is None or slot[0] != key:
            buf = None if slot is None or slot[1]["W1Tp"].device != fwd["W1p"].device else {n: slot[1][n] for n in ("W1Tp", "W2Tp")}
            with torch.no_grad():
                buf = ops.pack_moe_experts_backward([ex.lins[0].weight.detach() for ex in self.experts],
                                                    [ex.lins[1].weight.detach() for ex in self.experts], out=buf)
            self.__dict__["_packed_bwd"] = slot = (key, dict(fwd, **buf))
        return slot[1]

    def draw_noise(self, rows, device):
        """The standard-normal draws of noisy gating [rows, num_experts] (nn/moe.py:223), or None where the reference adds
        none: eval mode, or noisy_gating off."""
        if not (self.noisy_gating and self.training):
            return None
        return torch.randn(rows, self.num_experts, device=device, dtype=torch.float32)

    def sublayer(self, h, bn=None, noise=None, return_routing=False):
        """[BN_eval](h + MoE(h)) on the native kernels; noise: the draws to use instead of fresh ones (training mode)."""
        h = h.contiguous()
        if noise is None:
            noise = self.draw_noise(h.numel() // h.shape[-1], h.device)
        return ops.moe_ffn(h, self.w_gate.detach(), self.packed_experts(), self.k,
                           w_noise=self.w_noise.detach() if noise is not None else None, noise=noise, residual=h,
                           bn=bn, return_routing=return_routing)


class Normalization(nn.Module):
    def __init__(self, embed_dim, normalization="batch"):
        super().__init__()
        if normalization == "batch":
            self.normalizer = nn.BatchNorm1d(embed_dim, affine=True)
        elif normalization == "instance":
            self.normalizer = nn.InstanceNorm1d(embed_dim, affine=True)
        else:
            raise NotImplementedError(f"normalization={normalization!r}: only 'batch' and 'instance' are built for MI355X")

    def fused_bn(self):
        """(gamma, beta, mean, var, eps) when this is an eval-mode BatchNorm that the producing GEMM can apply;
        None for instance norm and for a BatchNorm in training mode (batch statistics: `apply_`)."""
        n = self.normalizer
        if not isinstance(n, nn.BatchNorm1d) or self.training:
            return None
        return (n.weight, n.bias, n.running_mean, n.running_var, n.eps)

    def apply_(self, x):
        n = self.normalizer
        if isinstance(n, nn.BatchNorm1d):
            if self.training:
                # batch statistics over all B*M rows, running statistics updated (nn/ops.py:45-47)
                momentum = 0.1 if n.momentum is None else n.momentum
                ops.batchnorm_train_(x, n.weight.detach(), n.bias.detach(), n.running_mean, n.running_var, momentum, n.eps)
                n.num_batches_tracked.add_(1)
                return x
            g, b, m, v, eps = self.fused_bn()
            return ops.normalize_(x, ops.NORM_BATCH_EVAL, g, b, m, v, eps)
        return ops.normalize_(x, ops.NORM_INSTANCE, n.weight, n.bias, eps=n.eps)


class MultiHeadAttentionLayer(nn.Sequential):
    """[SkipConnection(MHA), Normalization, SkipConnection(MLP), Normalization] (nn/graph/attnnet.py:16-57)."""

    def __init__(self, embed_dim, num_heads=8, feedforward_hidden=512, normalization="batch", bias=True, moe_kwargs=None):
        num_neurons = [feedforward_hidden] if feedforward_hidden > 0 else []
        ffn = MoE(embed_dim, embed_dim, num_neurons=num_neurons, **moe_kwargs) if moe_kwargs is not None \
            else _MLPParams(embed_dim, embed_dim, num_neurons)
        super().__init__(
            _Holder(_MHAParams(embed_dim, num_heads, bias=bias)),
            Normalization(embed_dim, normalization),
            _Holder(ffn),
            Normalization(embed_dim, normalization),
        )

    def forward(self, h):
        mha, ffn = self[0].module, self[2].module
        qkv = ops.linear(h, mha.Wqkv.weight, mha.Wqkv.bias)
        att = ops.mha_encoder(qkv, mha.num_heads)
        bn1, bn2 = self[1].fused_bn(), self[3].fused_bn()
        h = ops.linear(att, mha.out_proj.weight, mha.out_proj.bias, residual=h, bn=bn1)    # norm(h + MHA(h))
        if bn1 is None:
            h = self[1].apply_(h)
        if isinstance(ffn, MoE):
            h = ffn.sublayer(h, bn=bn2)                                                     # norm(h + MoE(h))
            return h if bn2 is not None else self[3].apply_(h)
        x = h
        for lin in ffn.lins[:-1]:
            x = ops.linear(x, lin.weight, lin.bias, relu=True)
        h = ops.linear(x, ffn.lins[-1].weight, ffn.lins[-1].bias, residual=h, bn=bn2)       # norm(h + FFN(h))
        return h if bn2 is not None else self[3].apply_(h)


class GraphAttentionNetwork(nn.Module):
    def __init__(self, num_heads, embed_dim, num_layers, normalization="batch", feedforward_hidden=512, moe_kwargs=None):
        super().__init__()
        self.layers = nn.Sequential(*(MultiHeadAttentionLayer(embed_dim, num_heads, feedforward_hidden, normalization,
                                                              moe_kwargs=moe_kwargs)
                                      for _ in range(num_layers)))
        self.dtype16 = None     # torch.float16 / torch.bfloat16: the fused kernel runs on 16-bit operands (policy.precision)

    def forward(self, x, mask=None, cache_spec=None, init=None, store_hidden=True, fused=None):
        """cache_spec (optional, from AttentionModelDecoder._fused_cache_spec): the fused kernel also fills the decoder cache
        from the embeddings it still holds in LDS and sets cache_spec["filled"].  init (instead of x; an init embedding's
        `fused_spec`, only with `fused` = this network's `_fused_layers`): the kernel computes the init embedding too and the
        call returns (embeddings or None when store_hidden is False, init embeddings or None)."""
        assert mask is None, "Mask not yet supported!"
        if fused is None:
            assert init is None, "init= needs the fused kernel (check _fused_layers first)"
            fused = self._fused_layers(x)
        if fused is not None:       # all layers of an instance in one workgroup, activations resident in LDS
            layers, H, ff, norm, eps, dtype = fused
            cache = None
            if cache_spec is not None:
                if cache_spec.get("dtype") != dtype:
                    raise RuntimeError("fused encoder: the decoder cache spec was packed for another precision")
                cache = (cache_spec["Wc"], cache_spec["WoT"], cache_spec["buf"], cache_spec["nproj"], cache_spec.get("Wg"),
                         cache_spec.get("gctx"))
            h = None if init is not None else x.contiguous()
            if dtype is None:
                out = ops.encoder_fused(h, layers, H, ff, norm, eps, cache=cache, init=init, store_hidden=store_hidden)
            else:
                out = ops.encoder_fused16(h, layers, H, ff, norm, eps, dtype, cache=cache, init=init, store_hidden=store_hidden)
            if cache_spec is not None:
                cache_spec["filled"] = True
            return out
        for layer in self.layers:
            x = layer(x)
        return x

    def _fused_layers(self, x, shape=None):
        """(layers, heads, ff_hidden, norm, eps, dtype): the arguments of `ops.encoder_fused` (dtype None) or
        `ops.encoder_fused16` (dtype = self.dtype16) when the fused kernel covers this network (eval-mode batch norm or
        instance norm, E = 128, 8 heads, one hidden layer of 512, graphs up to 112 nodes), else None.  The packed weights
        live in persistent buffers refreshed in place when a parameter changes (a captured HIP graph keeps reading them);
        16-bit packs have slots of their own per (layer, weight, dtype).  Outside that coverage (M > 112, batch norm in
        training mode, EAMRL_FUSED_ENCODER=0) the fp32 layer-by-layer path runs, whatever dtype16 says."""
        if os.environ.get("EAMRL_FUSED_ENCODER", "1") == "0" or len(self.layers) == 0:
            return None
        if any(isinstance(layer[2].module, MoE) for layer in self.layers):
            return None                 # MoE layers: the fp32 layer-by-layer path (ops.moe_ffn between its launches)
        first = self.layers[0]
        mha0, ffn0 = first[0].module, first[2].module
        if len(ffn0.lins) != 2:
            return None
        E, H, ff = mha0.embed_dim, mha0.num_heads, ffn0.lins[0].out_features
        if shape is None:       # shape = (M, E) of the embeddings when they are not materialised (fused init embedding)
            if x.dim() != 3:
                return None
            shape = (x.shape[1], x.shape[-1])
        if shape[1] != E or not ops.encoder_fused_supported(shape[0], E, H, ff, len(self.layers)):
            return None
        n0 = first[1].normalizer
        if isinstance(n0, nn.BatchNorm1d):
            if first[1].training:
                return None             # batch statistics: a reduction across instances (unfused path)
            norm = ops.NORM_BATCH_EVAL
        else:
            norm = ops.NORM_INSTANCE
        packed = self.__dict__.setdefault("_packed", {})
        dtype = self.dtype16
        out = []
        for li, layer in enumerate(self.layers):
            mha, ffn = layer[0].module, layer[2].module
            n1, n2 = layer[1].normalizer, layer[3].normalizer
            if (type(n1) is not type(n0) or type(n2) is not type(n0) or mha.num_heads != H or len(ffn.lins) != 2
                    or ffn.lins[0].out_features != ff or mha.Wqkv.bias is None or n1.eps != n0.eps or n2.eps != n0.eps):
                return None
            d = {}
            for name, lin in (("Wqkv", mha.Wqkv), ("Wo", mha.out_proj), ("W1", ffn.lins[0]), ("W2", ffn.lins[1])):
                w = lin.weight
                key = (w.data_ptr(), w._version, w.device)
                slot = packed.get((li, name) if dtype is None else (li, name, dtype))
                if slot is None or slot[0] != key:
                    buf = None if slot is None or slot[1].device != w.device else slot[1]
                    if dtype is None:
                        packed[(li, name)] = slot = (key, ops.pack_linear_weight(w.detach().contiguous(), out=buf))
                    else:
                        packed[(li, name, dtype)] = slot = (key, ops.pack_linear_weight16(w.detach().contiguous(), dtype, out=buf))
                d[name] = slot[1]
            d.update(bqkv=mha.Wqkv.bias.detach(), bo=mha.out_proj.bias.detach(), b1=ffn.lins[0].bias.detach(),
                     b2=ffn.lins[1].bias.detach(), n1_gamma=n1.weight.detach(), n1_beta=n1.bias.detach(),
                     n2_gamma=n2.weight.detach(), n2_beta=n2.bias.detach())
            if norm == ops.NORM_BATCH_EVAL:
                d.update(n1_mean=n1.running_mean, n1_var=n1.running_var, n2_mean=n2.running_mean, n2_var=n2.running_var)
            out.append(d)
        return out, H, ff, norm, n0.eps, dtype


class AttentionModelEncoder(nn.Module):
    def __init__(self, embed_dim=128, init_embedding=None, env_name="tsp", num_heads=8, num_layers=3,
                 normalization="batch", feedforward_hidden=512, net=None, sdpa_fn=None, moe_kwargs=None):
        super().__init__()
        env_name = _kind(env_name)
        if sdpa_fn is not None:
            raise NotImplementedError("sdpa_fn injection is outside the MI355X rollout path")
        if moe_kwargs is not None and net is not None:
            raise NotImplementedError("moe_kwargs with net=: the MoE sublayer is built into GraphAttentionNetwork; pass "
                                      "GraphAttentionNetwork(..., moe_kwargs=...) as the net")
        self.env_name = env_name
        if init_embedding is None:
            init_embedding = {"tsp": TSPInitEmbedding, "cvrp": VRPInitEmbedding, "sdvrp": VRPInitEmbedding,
                              "pctsp": PCTSPInitEmbedding, "op": OPInitEmbedding,
                              "cvrptw": VRPTWInitEmbedding, "pdp": PDPInitEmbedding}[env_name](embed_dim)
        self.init_embedding = init_embedding
        self.net = GraphAttentionNetwork(num_heads, embed_dim, num_layers, normalization, feedforward_hidden,
                                         moe_kwargs=moe_kwargs) if net is None else net

    def forward(self, td, mask=None, cache_spec=None, want_hidden=True, want_init=True):
        """-> (embeddings, init embeddings).  With a `cache_spec` the whole encoder can be ONE launch that starts from the
        node features (`init_embedding.fused_spec`) and ends in the decoder cache; want_hidden / want_init = False then
        return None for tensors the caller does not need (they never leave the workgroup's LDS)."""
        spec_fn = getattr(self.init_embedding, "fused_spec", None)
        if (cache_spec is not None and spec_fn is not None and mask is None and isinstance(self.net, GraphAttentionNetwork)
                and os.environ.get("EAMRL_FUSED_INIT", "1") != "0"):
            M, E = td["locs"].shape[1], self.net.layers[0][0].module.embed_dim if len(self.net.layers) else 0
            fused = self.net._fused_layers(None, (M, E)) if E else None
            init = spec_fn(td) if fused is not None else None
            if init is not None:
                init["want_init"] = want_init
                return self.net(None, None, cache_spec=cache_spec, init=init, store_hidden=want_hidden, fused=fused)
        init_h = self.init_embedding(td)
        h = self.net(init_h, mask, cache_spec=cache_spec) if cache_spec is not None else self.net(init_h, mask)
        return h, init_h


# ------------------------------------------------------------------------------------------------------------
# Heterogeneous Attention Model (HAM) encoder for pickup and delivery (zoo/ham/{attention,encoder,policy}.py)
# ------------------------------------------------------------------------------------------------------------
class HeterogenousMHA(nn.Module):
    """Parameters of the reference's HeterogenousMHA (zoo/ham/attention.py:7-51, its spelling): W_query, W_key, W_val and the
    six role queries W1..W6 as [H, E, D], W_out as [H, D, E], no biases, the reference's uniform(+-1/sqrt(last dim)) init.
    `forward` is projections (eamrl_linear on the packed weights), eamrl_hetero_mha, W_out."""

    def __init__(self, num_heads, input_dim, embed_dim=None, val_dim=None, key_dim=None):
        super().__init__()
        if val_dim is None and embed_dim is None:
            raise ValueError("HeterogenousMHA: give embed_dim (head width = embed_dim // num_heads) or val_dim")
        head = embed_dim // num_heads if val_dim is None else val_dim
        key_dim = head if key_dim is None else key_dim
        if embed_dim != input_dim or key_dim != head or num_heads * head != input_dim:
            raise NotImplementedError("HeterogenousMHA: only embed_dim = input_dim = num_heads * key_dim (= val_dim) is built "
                                      "for MI355X (the HAM encoder's configuration)")
        self.num_heads, self.input_dim, self.embed_dim, self.val_dim, self.key_dim = num_heads, input_dim, embed_dim, head, key_dim
        self.norm_factor = key_dim ** -0.5
        for name in ("W_query", "W_key", "W_val", "W1_query", "W2_query", "W3_query", "W4_query", "W5_query", "W6_query"):
            setattr(self, name, nn.Parameter(torch.empty(num_heads, input_dim, key_dim)))
        self.W_out = nn.Parameter(torch.empty(num_heads, key_dim, embed_dim))
        self.init_parameters()

    def init_parameters(self):
        """Uniform in +-1/sqrt(last dimension), the reference's distribution.  Through nn.init, so that the version counters
        move and `packed()` sees a later re-initialisation."""
        with torch.no_grad():
            for w in self.parameters():
                nn.init.uniform_(w, -w.shape[-1] ** -0.5, w.shape[-1] ** -0.5)

    PACKS = (("qkv", ("W_query", "W_key", "W_val")), ("pick", ("W1_query", "W2_query", "W3_query")),
             ("deliv", ("W4_query", "W5_query", "W6_query")))

    def packed(self):
        """{"qkv", "pick", "deliv": [3E, E] Linear weights ([(h d), E] per projection, stacked), "out": [E, E] = W_out.view(H D,
        E) transposed}: persistent buffers, repacked IN PLACE when a parameter's (data_ptr, _version) changes (a captured HIP
        graph keeps reading them), as GraphAttentionNetwork._fused_layers keeps its packs."""
        slots = self.__dict__.setdefault("_packed", {})
        E = self.input_dim
        out = {}
        for name, keys in self.PACKS + (("out", ("W_out",)),):
            ws = [getattr(self, k) for k in keys]
            key = tuple((w.data_ptr(), w._version, w.device) for w in ws)
            slot = slots.get(name)
            if slot is None or slot[0] != key:
                with torch.no_grad():
                    if name == "out":
                        new = ws[0].detach().reshape(-1, self.embed_dim).t()                    # [E, (h d)]
                    else:
                        new = torch.cat([w.detach().permute(0, 2, 1).reshape(-1, E) for w in ws], 0)      # [3 (h d), E]
                    if slot is not None and slot[1].device == new.device and slot[1].shape == new.shape:
                        slot[1].copy_(new)
                        slots[name] = slot = (key, slot[1])
                    else:
                        slots[name] = slot = (key, new.contiguous())
            out[name] = slot[1]
        return out

    def project(self, h):
        """proj [B, M, 6E] = q | k | v | qpair | qsame | qother by three GEMMs: all nodes on the stacked W_query | W_key | W_val,
        the pickups on W1 | W2 | W3, the deliveries on W4 | W5 | W6.  The role rows of a batch have no single row stride, so
        they are gathered role-major ([2, B, P, E], one copy) and the role queries scattered back (one copy).  The depot's last
        3E stay unwritten: the kernel never reads them."""
        B, M, E = h.shape
        assert M % 2 == 1, ops.ODD_NODES_MESSAGE
        assert E == self.input_dim, "Wrong embedding dimension of input"
        P = (M - 1) // 2
        w = self.packed()
        proj = torch.empty(B, M, 6 * E, device=h.device, dtype=torch.float32)
        ops.linear(h, w["qkv"], out=proj.view(B * M, 6 * E)[:, 0:3 * E])
        if B * P:
            roles = h[:, 1:].view(B, 2, P, E).permute(1, 0, 2, 3).contiguous()                  # [2, B, P, E]
            extra = torch.empty(2, B, P, 3 * E, device=h.device, dtype=torch.float32)
            ops.linear(roles[0], w["pick"], out=extra[0])
            ops.linear(roles[1], w["deliv"], out=extra[1])
            proj[:, 1:, 3 * E:].view(B, 2, P, 3 * E).copy_(extra.permute(1, 0, 2, 3))
        return proj

    def forward(self, q, h=None, mask=None):
        if h is not None or mask is not None:
            raise NotImplementedError("HeterogenousMHA: self-attention without a mask only (what the HAM encoder calls)")
        att = ops.hetero_mha(self.project(q.contiguous()), self.num_heads)
        return ops.linear(att, self.packed()["out"])


class HeterogeneuousMHALayer(nn.Sequential):
    """[SkipConnection(HeterogenousMHA), Normalization, SkipConnection(FFN), Normalization] (zoo/ham/encoder.py:8-29, its
    spelling).  The FFN is an nn.Sequential(Linear, ReLU, Linear) holder so that the keys are `.2.module.0.*` / `.2.module.2.*`."""

    def __init__(self, num_heads, embed_dim, feedforward_hidden=512, normalization="batch"):
        super().__init__(
            _Holder(HeterogenousMHA(num_heads, embed_dim, embed_dim)),
            Normalization(embed_dim, normalization),
            _Holder(nn.Sequential(nn.Linear(embed_dim, feedforward_hidden), nn.ReLU(), nn.Linear(feedforward_hidden, embed_dim))
                    if feedforward_hidden > 0 else nn.Linear(embed_dim, embed_dim)),
            Normalization(embed_dim, normalization),
        )

    def forward(self, h):
        mha, ffn = self[0].module, self[2].module
        att = ops.hetero_mha(mha.project(h), mha.num_heads)
        bn1, bn2 = self[1].fused_bn(), self[3].fused_bn()
        h = ops.linear(att, mha.packed()["out"], None, residual=h, bn=bn1)                 # norm(h + MHA(h))
        if bn1 is None:
            h = self[1].apply_(h)
        if isinstance(ffn, nn.Linear):
            return self._finish(ops.linear(h, ffn.weight, ffn.bias, residual=h, bn=bn2), bn2)
        x = ops.linear(h, ffn[0].weight, ffn[0].bias, relu=True)
        return self._finish(ops.linear(x, ffn[2].weight, ffn[2].bias, residual=h, bn=bn2), bn2)     # norm(h + FFN(h))

    def _finish(self, h, bn2):
        return h if bn2 is not None else self[3].apply_(h)


class GraphHeterogeneousAttentionEncoder(nn.Module):
    """zoo/ham/encoder.py:32-73: init embedding + HeterogeneuousMHALayer x num_encoder_layers -> (embeddings, init embeddings)."""

    def __init__(self, init_embedding=None, num_heads=8, embed_dim=128, num_encoder_layers=3, env_name=None,
                 normalization="batch", feedforward_hidden=512, sdpa_fn=None):
        super().__init__()
        if sdpa_fn is not None:
            raise NotImplementedError("sdpa_fn injection is outside the MI355X rollout path")
        env_name = "pdp" if env_name is None else _kind(env_name)
        if init_embedding is None:
            if env_name != "pdp":
                raise NotImplementedError(f"GraphHeterogeneousAttentionEncoder: env_name={env_name!r}; the heterogeneous attention "
                                          "is defined for pickup and delivery ('pdp')")
            init_embedding = PDPInitEmbedding(embed_dim)
        self.env_name = env_name
        self.init_embedding = init_embedding
        self.layers = nn.Sequential(*(HeterogeneuousMHALayer(num_heads, embed_dim, feedforward_hidden, normalization)
                                      for _ in range(num_encoder_layers)))

    def forward(self, x, mask=None):
        assert mask is None, "Mask not yet supported!"
        init_embeds = self.init_embedding(x)
        h = init_embeds
        for layer in self.layers:
            h = layer(h)
        return h, init_embeds

    def refresh_packs(self):
        """Repack weights that changed into the buffers a captured graph reads (GraphedRollout)."""
        for layer in self.layers:
            layer[0].module.packed()


class _ContextParams(nn.Module):
    def __init__(self, embed_dim, step_context_dim, placeholder):
        super().__init__()
        self.embed_dim = embed_dim
        self.project_context = nn.Linear(step_context_dim, embed_dim, bias=False)
        if placeholder:
            self.W_placeholder = nn.Parameter(torch.Tensor(2 * embed_dim).uniform_(-1, 1))


class _PointerParams(nn.Module):
    def __init__(self, embed_dim, num_heads, mask_inner=True, out_bias=False, check_nan=True):
        super().__init__()
        if not mask_inner or out_bias:
            raise NotImplementedError("mask_inner=False / out_bias_pointer_attn=True are not built for MI355X")
        self.num_heads, self.mask_inner, self.check_nan = num_heads, mask_inner, check_nan
        self.project_out = nn.Linear(embed_dim, embed_dim, bias=False)


class StaticEmbedding(nn.Module):
    def forward(self, td):
        return 0, 0, 0


class SDVRPDynamicEmbedding(nn.Module):
    """Parameters of the SDVRP dynamic embedding (nn/env_embeddings/dynamic.py:59-78): Linear(1, 3E) of the remaining
    demand, added to the cached glimpse key / value / logit key at every step (inside the decode kernels)."""

    def __init__(self, embed_dim, linear_bias=False):
        super().__init__()
        if linear_bias:
            raise NotImplementedError("SDVRPDynamicEmbedding with bias is not built for MI355X")
        self.projection = nn.Linear(1, 3 * embed_dim, bias=False)


class AttentionModelDecoder(nn.Module):
    """Pointer decoder.  `_precompute_cache` is the one-shot part (GEMMs), `forward` one decode step."""

    def __init__(self, embed_dim=128, num_heads=8, env_name="tsp", context_embedding=None, dynamic_embedding=None,
                 mask_inner=True, out_bias_pointer_attn=False, linear_bias=False, use_graph_context=True,
                 check_nan=True, sdpa_fn=None, pointer=None, moe_kwargs=None):
        super().__init__()
        env_name = _kind(env_name)
        from .attention import PointerAttention

        if pointer is not None and not (isinstance(pointer, PointerAttention) and pointer.project_out.bias is None
                                        and pointer.mask_inner and pointer.num_heads == num_heads):
            raise NotImplementedError("pointer=: only eam_rl4co_amd.PointerAttention (mask_inner, no output bias, the decoder's "
                                      "head count) can replace the built-in pointer; its project_out is what the fused "
                                      "kernels fold into the logit key")
        if moe_kwargs is not None:
            raise NotImplementedError("moe_kwargs['decoder'] (PointerAttnMoE, light or not) is not built: only the encoder half of "
                                      "MVMoE is (moe_kwargs['encoder']); a per-row project_out breaks the folded logit key of the "
                                      "one-launch rollout")
        if any(x is not None for x in (context_embedding, dynamic_embedding, sdpa_fn)) or linear_bias:
            raise NotImplementedError("custom context/dynamic embeddings, sdpa_fn and decoder biases are "
                                      "outside the MI355X rollout path (the routing AttentionModel family only)")
        assert embed_dim % num_heads == 0
        self.env_name, self.embed_dim, self.num_heads = env_name, embed_dim, num_heads
        # node(s) + state columns; PDPContext (context.py:242-253) is the current node alone: a square project_context
        ctx_dim = {"tsp": 2 * embed_dim, "cvrptw": embed_dim + 2, "pdp": embed_dim}.get(env_name, embed_dim + 1)
        self.context_embedding = _ContextParams(embed_dim, ctx_dim, placeholder=(env_name == "tsp"))
        self.dynamic_embedding = SDVRPDynamicEmbedding(embed_dim) if env_name == "sdvrp" else StaticEmbedding()
        self.is_dynamic_embedding = env_name == "sdvrp"
        self.pointer = pointer if pointer is not None else _PointerParams(embed_dim, num_heads, mask_inner,
                                                                          out_bias_pointer_attn, check_nan)
        self.project_node_embeddings = nn.Linear(embed_dim, 3 * embed_dim, bias=False)
        self.project_fixed_context = nn.Linear(embed_dim, embed_dim, bias=False)
        self.use_graph_context = use_graph_context

    def _fused_cache_spec(self, B: int, M: int, device, dtype=None):
        """What the fused encoder kernel needs to fill the slot-major cache itself (K | V | L | Pa (| Pb) projections of the
        final embeddings + Lp = L Wout), or None where that layout is not used (graphs above 128 nodes: plane-major).
        dtype (torch.float16 / torch.bfloat16): Wc / WoT are the 16-bit packs of the 16-bit fused encoder."""
        if M > 128 or os.environ.get("EAMRL_FUSED_CACHE", "1") == "0":
            return None
        E = self.embed_dim
        self._weight_constants()
        slots = ops.slot_map(self.env_name)
        nproj = len(slots) - 1      # K, V, L, Pa (, Pb): all but Lp
        Wout = self.pointer.project_out.weight
        key = (self._wc_key, Wout.data_ptr(), Wout._version)
        if dtype is not None:       # 16-bit packs: slots of their own per dtype, refreshed in place like the fp32 ones
            fc16 = self.__dict__.setdefault("_fc16", {})
            old = fc16.get(dtype)
            if old is None or old[0] != key:
                keep = old is not None and old[1].device == self._w_cache.device and old[1].numel() == self._w_cache.numel()
                Wc = ops.pack_linear_weight16(self._w_cache, dtype, out=old[1] if keep else None)
                WoT = ops.pack_linear_weight16(Wout.detach().t().contiguous(), dtype, out=old[2] if keep else None)
                fc16[dtype] = (key, Wc, WoT)
            packs = fc16[dtype][1:]
        else:
            if getattr(self, "_fc_key", None) != key:
                old = getattr(self, "_fc", None)
                keep = old is not None and old[0].device == self._w_cache.device and old[0].numel() == self._w_cache.numel()
                Wc = ops.pack_linear_weight(self._w_cache, out=old[0] if keep else None)
                WoT = ops.pack_linear_weight(Wout.detach().t().contiguous(), out=old[1] if keep else None)
                self._fc, self._fc_key = (Wc, WoT), key
            packs = self._fc
        buf = torch.empty(B, M, len(slots) * E, device=device, dtype=torch.float32)
        spec = {"buf": buf, "Wc": packs[0], "WoT": packs[1], "nproj": nproj, "filled": False, "dtype": dtype}
        Wg = self.project_fixed_context.weight if self.use_graph_context else None
        if Wg is not None and Wg.is_contiguous() and Wg.data_ptr() % 16 == 0 and B > 0:     # the live parameter: nothing to refresh
            spec["Wg"], spec["gctx"] = Wg.detach(), torch.empty(B, E, device=device, dtype=torch.float32)
        return spec

    def _precompute_cache(self, embeddings: torch.Tensor, num_starts: int = 0, prefilled=None) -> ops.DecodeCache:
        """K | V | L (+ folded context / logit projections) in one slot-major buffer (ops.DecodeCache).  prefilled: a
        `_fused_cache_spec` whose buffer the fused encoder kernel has already filled (only the graph context is left)."""
        E = self.embed_dim
        slots = ops.slot_map(self.env_name)
        Wa, Wb, cvec = self._weight_constants()
        Wkvl = self.project_node_embeddings.weight
        if embeddings is None:      # the fused encoder kept them in LDS: everything derived from them is already in `prefilled`
            assert prefilled is not None and prefilled.get("filled") and (not self.use_graph_context or prefilled.get("gctx") is not None)
            emb = None
        else:
            emb = embeddings.contiguous()
            B, M, _ = emb.shape
        if prefilled is not None and prefilled.get("filled"):
            buf = prefilled["buf"]
        elif M > 128 and os.environ.get("EAMRL_CACHE_PLANES", "1") != "0":     # streaming-kernel territory: one dense
            # plane per kind of row (ops.DecodeCache); the variable exists for A/B measurements only
            buf = torch.empty(len(slots), B, M, E, device=emb.device, dtype=torch.float32)
            plane = lambda n: buf[slots[n]].view(B * M, E)
            for i, n in enumerate(("K", "V", "L")):
                ops.linear(emb, Wkvl[i * E:(i + 1) * E], out=plane(n))
            ops.linear(emb, Wa, out=plane("Pa"))
            if self.env_name == "tsp":
                ops.linear(emb, Wb, out=plane("Pb"))
            ops.matmul_right(plane("L"), self.pointer.project_out.weight.contiguous(), out=plane("Lp"))
        else:
            buf = torch.empty(B, M, len(slots) * E, device=emb.device, dtype=torch.float32)
            flat = buf.view(B * M, -1)
            nproj = len(slots) - 1          # K, V, L, Pa (, Pb): slots 0 .. nproj-1, all but Lp
            assert slots["Pa"] == 3 and slots.get("Pb", 4) == 4
            ops.linear(emb, self._w_cache, out=flat[:, 0:nproj * E])
            ops.matmul_right(flat[:, slots["L"] * E:(slots["L"] + 1) * E], self.pointer.project_out.weight.contiguous(),
                             out=flat[:, slots["Lp"] * E:(slots["Lp"] + 1) * E])
        gctx = None
        if self.use_graph_context:
            if prefilled is not None and prefilled.get("filled") and prefilled.get("gctx") is not None:
                gctx = prefilled["gctx"]                  # written by the fused encoder kernel
            else:
                gctx = ops.linear(ops.mean_nodes(emb), self.project_fixed_context.weight)
        dyn = None
        if self.is_dynamic_embedding:       # key and value columns as they are; the logit-key column times project_out
            w = self.dynamic_embedding.projection.weight.detach().reshape(3, E)
            lw = ops.matmul_right(w[2:3].contiguous(), self.pointer.project_out.weight.contiguous())
            dyn = torch.cat((w[0:2], lw), 0).contiguous()
        return ops.DecodeCache(self.env_name, buf, None if cvec is None else cvec.contiguous(), gctx, emb, self.num_heads,
                               dyn=dyn, embed_dim=E)

    def _weight_constants(self):
        """Tensors that depend on the weights only, recomputed when a parameter changes (optimizer step, load):
        the two halves of project_context as contiguous matrices (aligned float4 rows for the GEMM) and the
        constant part of the query (TSP: project_context(W_placeholder); CVRP: the capacity column)."""
        E = self.embed_dim
        Wctx = self.context_embedding.project_context.weight
        ph = getattr(self.context_embedding, "W_placeholder", None)
        Wkvl = self.project_node_embeddings.weight
        key = (Wctx.data_ptr(), Wctx._version, None if ph is None else (ph.data_ptr(), ph._version),
               Wkvl.data_ptr(), Wkvl._version)
        if getattr(self, "_wc_key", None) != key:
            Wa = Wctx[:, 0:E].contiguous()
            if self.env_name == "tsp":
                Wb = Wctx[:, E:2 * E].contiguous()
                cvec = ops.linear(ph[None, :].detach(), Wctx.detach())[0].contiguous()
            else:
                Wb = None
                # state columns: capacity (CVRP-like), prize / length left (PCTSP / OP); CVRPTW: capacity | time -> [2E]
                cvec = (None if self.env_name == "pdp" else          # PDP: no state column (eamrl_cache.cvec = NULL)
                        Wctx[:, E:].t().reshape(-1).contiguous() if self.env_name == "cvrptw" else Wctx[:, E].contiguous())
            # slot-major cache: K | V | L | Pa (| Pb) are adjacent slots, so one GEMM with the stacked weights writes them all
            # (each output element is the same k-ordered chain as with separate launches)
            w_cache = torch.cat([Wkvl.detach(), Wa.detach()] + ([Wb.detach()] if Wb is not None else []), 0).contiguous()
            new = (Wa.detach(), None if Wb is None else Wb.detach(), None if cvec is None else cvec.detach())
            old = getattr(self, "_wc", None)
            if old is not None and all((a is None) == (b is None) and (a is None or (a.shape == b.shape and a.device == b.device))
                                       for a, b in zip(old, new)) and self._w_cache.shape == w_cache.shape:
                # refresh IN PLACE: a captured HIP graph (GraphedRollout) holds pointers to these buffers
                for a, b in zip(old, new):
                    if a is not None:
                        a.copy_(b)
                self._w_cache.copy_(w_cache)
            else:
                self._wc, self._w_cache = new, w_cache
            self._wc_key = key
        return self._wc

    def pre_decoder_hook(self, td, env, embeddings, num_starts: int = 0):
        return td, env, self._precompute_cache(embeddings, num_starts=num_starts)

    def forward(self, td, cached: ops.DecodeCache, num_starts: int = 0):
        """(logits, mask) for the current state, as the reference decoder returns them (decoder.py:161-198)."""
        st = state_from_td(self.env_name, td, copy=False)      # read-only: the step is not fused
        _, _, _, logits, status = ops.decode_step(st, cached, "greedy", clip=0.0, temp=1.0, want_logits=True)
        if self.pointer.check_nan:
            ops.raise_on_status(int(status.item()) & ops.ST_NAN_LOGITS)
        return logits, td["action_mask"]


def _env_step_(st: ops.RolloutState, action):
    """The env transition (+ mask) of `st.env_name` on the flat state, in place."""
    fn, args = ENV_SPECS[st.env_name].step
    getattr(ops, fn)(*(action if a == ACTION else a if a is None else getattr(st, a) for a in args))


_max_decode_steps = max_steps        # (env_name, M, npre=0): the bound of the env's record


# ------------------------------------------------------------------------------------------------------------
# TensorDict <-> flat rollout state
# ------------------------------------------------------------------------------------------------------------
def state_from_td(env_name, td, num_starts: int = 0, copy: bool = True) -> ops.RolloutState:
    """Flat state tensors for R = max(S,1)*B rows, replicated in the reference's (s b) order for multistart
    (utils/ops.py:13-33 batchify).  The kernels update the state in place, so the tensors are copies: like the
    reference's rollout, a policy call leaves the caller's TensorDict as it was (the same td can be rolled out again,
    e.g. by a rollout baseline).  copy=False hands out views of the td's own tensors (read-only uses).
    Which key lands in which slot, as what: env_spec.ENV_SPECS[env_name].fields."""
    mask = td["action_mask"]
    B, M = mask.shape
    S = max(int(num_starts), 1)
    dev = mask.device
    if not mask.is_cuda:
        raise RuntimeError(f"TensorDict is on {dev}: the eam_rl4co_amd rollout path runs only on an MI355X (HIP) "
                           "device; there is no CPU fallback. Use td.to('cuda').")
    st = ops.RolloutState.__new__(ops.RolloutState)
    st.env_name, st.R, st.M = env_name, B * S, M
    clones = []                                           # (dst, src): all clones of a call go out as ONE launch

    def rep(t, dtype):
        src = t
        t = t.reshape(B, -1) if t.dim() > 1 else t.reshape(B)
        if t.dtype != dtype:
            t = t.to(dtype)
        if S > 1:
            t = t.repeat(S, *([1] * (t.dim() - 1)))
        elif copy and t.data_ptr() == src.data_ptr():     # still the caller's storage
            if t.is_contiguous():
                dst = torch.empty_like(t)
                clones.append((dst, t))
                t = dst
            else:
                t = t.clone()
        t = t.contiguous()
        return t.reshape(-1) if t.dim() == 2 and t.shape[1] == 1 else t

    st.mask = rep(mask, torch.bool)
    done = td["done"] if "done" in td.keys() else torch.zeros(B, dtype=torch.bool, device=dev)
    st.done = rep(done, torch.bool)
    for f in ENV_SPECS[env_name].fields:
        t = td[f.key]
        t = t[..., 0] if f.transform == "col0" else ~t if f.transform == "not" else t
        setattr(st, f.slot, rep(t, f.dtype) if f.per_row else (t if t.dtype == f.dtype else t.to(f.dtype)).contiguous())
    if clones:
        ops.multi_copy_(clones)
    return st


def state_to_td(env_name, st: ops.RolloutState, td, locs_rows=None):
    """TensorDict of the final state in the reference's post-step shapes."""
    R = st.R
    out = {"action_mask": st.mask, "done": st.done, "reward": torch.zeros_like(st.done)}
    for f in ENV_SPECS[env_name].fields:
        if f.per_row and f.emit:
            v = getattr(st, f.slot)
            v = v == 0 if f.transform == "not" else v != 0 if f.src_dtype == torch.bool else v
            out[f.key] = v.reshape(R, 1) if f.shape == (1,) else v     # (the state's scalars are flat [R])
    B = td.batch_size[0]
    S = R // B
    for k, v in td.items():
        if k in out or k == "action":
            continue
        out[k] = v if S == 1 else v.repeat(S, *([1] * (v.dim() - 1)))
    return TensorDict(out, batch_size=[R])


# ------------------------------------------------------------------------------------------------------------
# the policy
# ------------------------------------------------------------------------------------------------------------
class AttentionModelPolicy(nn.Module):
    """Kool et al. (2019) attention model; see module docstring.  Constructor arguments follow
    rl4co/models/zoo/am/policy.py:50-122 (unsupported injections raise NotImplementedError)."""

    def __init__(self, encoder: nn.Module = None, decoder: nn.Module = None, embed_dim: int = 128,
                 num_encoder_layers: int = 3, num_heads: int = 8, normalization: str = "batch",
                 feedforward_hidden: int = 512, env_name: str = "tsp", encoder_network: nn.Module = None,
                 init_embedding: nn.Module = None, context_embedding: nn.Module = None,
                 dynamic_embedding: nn.Module = None, use_graph_context: bool = True,
                 linear_bias_decoder: bool = False, sdpa_fn=None, sdpa_fn_encoder=None, sdpa_fn_decoder=None,
                 mask_inner: bool = True, out_bias_pointer_attn: bool = False, check_nan: bool = True,
                 temperature: float = 1.0, tanh_clipping: float = 10.0, mask_logits: bool = True,
                 train_decode_type: str = "sampling", val_decode_type: str = "greedy",
                 test_decode_type: str = "greedy", moe_kwargs: dict = None, precision: str = "32-true", **unused_kwargs):
        super().__init__()
        if unused_kwargs:
            log.error("Found %d unused kwargs: %s", len(unused_kwargs), unused_kwargs)
        if isinstance(env_name, RL4COEnvBase):
            env_name = env_name.name
        self.env_alias = env_name            # the name the env must carry (e.g. "spctsp")
        env_name = _kind(env_name)           # the kernel / embedding family (e.g. "pctsp")
        if env_name not in ("tsp", "cvrp", "cvrptw", "sdvrp", "pctsp", "op", "pdp"):
            raise NotImplementedError(f"env_name={env_name!r}: the MI355X rollout path covers 'tsp', 'cvrp', 'cvrptw', 'pdp', "
                                      "'sdvrp', 'pctsp', 'spctsp' and 'op'")
        if any(x is not None for x in (sdpa_fn, sdpa_fn_encoder, sdpa_fn_decoder, encoder_network)):
            raise NotImplementedError("sdpa_fn / encoder_network injection is outside the MI355X rollout path")
        moe_kwargs = {"encoder": None, "decoder": None} if moe_kwargs is None else moe_kwargs
        if moe_kwargs.get("decoder") is not None:
            raise NotImplementedError("moe_kwargs['decoder'] (PointerAttnMoE, light or not) is not built: only the encoder half of "
                                      "MVMoE is (moe_kwargs['encoder'])")
        if moe_kwargs.get("encoder") is not None and encoder is not None:
            raise NotImplementedError("moe_kwargs['encoder'] with encoder=: build the encoder with its own moe_kwargs")
        if not mask_logits:
            raise NotImplementedError("mask_logits=False is not built for MI355X")
        self.env_name = env_name
        self.encoder = encoder if encoder is not None else AttentionModelEncoder(
            embed_dim=embed_dim, num_heads=num_heads, num_layers=num_encoder_layers, env_name=env_name,
            normalization=normalization, feedforward_hidden=feedforward_hidden, init_embedding=init_embedding,
            moe_kwargs=moe_kwargs.get("encoder"))
        self.decoder = decoder if decoder is not None else AttentionModelDecoder(
            embed_dim=embed_dim, num_heads=num_heads, env_name=env_name, context_embedding=context_embedding,
            dynamic_embedding=dynamic_embedding, mask_inner=mask_inner, out_bias_pointer_attn=out_bias_pointer_attn,
            linear_bias=linear_bias_decoder, use_graph_context=use_graph_context, check_nan=check_nan)
        self.temperature, self.tanh_clipping, self.mask_logits = temperature, tanh_clipping, mask_logits
        self.train_decode_type, self.val_decode_type, self.test_decode_type = (
            train_decode_type, val_decode_type, test_decode_type)
        self.precision = precision

    @property
    def precision(self) -> str:
        """Operand precision of the fused encoder in rollouts that build no autograd graph, by Lightning's names:
        "32-true" (default, fp32 MFMA, bit-exact), "16-mixed" (fp16 operands) or "bf16-mixed" (bf16 operands), fp32
        accumulation either way.  A plain attribute: not in the state_dict, kept by copy.deepcopy.
        Training (forward with autograd in phase "train") needs "32-true"."""
        return self.__dict__["_precision"]

    @precision.setter
    def precision(self, value: str):
        if value not in PRECISIONS:
            raise ValueError(f"precision={value!r}: expected one of {sorted(PRECISIONS)}")
        dtype = PRECISIONS[value]
        net = getattr(self.encoder, "net", None)
        if isinstance(net, GraphAttentionNetwork):
            net.dtype16 = dtype
        elif dtype is not None:
            raise NotImplementedError("precision: 16-bit operands need the built-in GraphAttentionNetwork encoder")
        self.__dict__["_precision"] = value

    @property
    def _dtype16(self):
        return PRECISIONS[self.__dict__["_precision"]]

    def forward(self, td, env: Optional[str | RL4COEnvBase] = None, phase: str = "train", calc_reward: bool = True,
                return_actions: bool = True, return_entropy: bool = False, return_hidden: bool = False,
                return_init_embeds: bool = False, return_sum_log_likelihood: bool = True, actions=None,
                max_steps=1_000_000, **decoding_kwargs) -> dict:
        """The construction rollout (constructive/base.py:157-275): encode once, precompute the cache, run the
        whole decode loop on the device, compute reward and log-likelihood.
        Two halves: `_enqueue` launches every kernel without touching the host (it can be captured into a HIP
        graph, see GraphedRollout), `_finish` performs the rollout's single device->host sync and slices.

        Gradients: the kernels build no graph.  With autograd enabled and phase == "train" (what REINFORCE / POMO /
        EAM.shared_step call, reinforce.py:62-64, pomo/model.py:103, earl/model.py:179-195) the returned
        `log_likelihood` carries a grad_fn: its value is the native rollout's, its gradient is that of the
        teacher-forced re-evaluation of the chosen actions (train.attach_log_likelihood_grad), so
        `loss = -(advantage * out["log_likelihood"]).mean(); loss.backward()` works as with the reference.  Validation /
        test phases run under no_grad in the reference's trainers and are not re-evaluated here."""
        want_grad = (torch.is_grad_enabled() and phase == "train" and not torch.is_inference_mode_enabled()
                     and any(q.requires_grad for q in self._parameter_list()))
        if want_grad and self._dtype16 is not None:
            raise NotImplementedError(f"precision={self.precision!r}: 16-bit training is not built (the backward re-uses the "
                                      "rollout's log-probabilities, which need the fp32 encoder); use precision='32-true', "
                                      "or run the rollout under torch.no_grad()")
        self._want_heads = want_grad and os.environ.get("EAMRL_REEVAL_RECOMPUTE_HEADS", "0") != "1"
        own_shared = False
        try:
            if want_grad:
                own_shared = self._one_encoder_pass(td, return_init_embeds)
            with torch.no_grad():
                try:
                    p = self._enqueue(td, env, phase, calc_reward, return_actions, return_entropy, return_hidden,
                                      return_init_embeds, return_sum_log_likelihood, actions, max_steps, **decoding_kwargs)
                finally:
                    self._want_heads = False        # (GraphedRollout calls _enqueue directly)
                if "out" in p:          # beam search is host-driven and arrives finished (inference only)
                    return p["out"]
                p["given_actions"] = actions is not None
                out = self._finish(p)
            return self._attach_grad(out, p) if want_grad else out
        finally:
            if own_shared:
                self._shared_dt = None

    def _pointer_operands(self):
        """Extra weight operands of the decode kernels' pointer (ops.rollout's `poly`): none for the plain pointer."""
        return None

    def _parameter_list(self):
        """The Parameter objects, kept: walking the module tree costs 0.3 ms and every forward asks (see train._graph_key)."""
        lists = self.__dict__.get("_key_tensors")
        if lists is None:
            lists = (list(self.parameters()), list(self.buffers()))
            self.__dict__["_key_tensors"] = lists
        return lists[0]

    def _has_moe(self) -> bool:
        from .train import has_moe_encoder

        return has_moe_encoder(self)

    def _one_encoder_pass(self, td, return_init_embeds) -> bool:
        """Training: where the differentiable encoder of the gradient graph reproduces the native encoder bit for bit
        (train.graph_encoder_equals_native), it is built FIRST and its embeddings feed the rollout -- one encoder pass per step
        instead of the fused kernel for the rollout plus the graph's own forward.  The graph and the embeddings are handed
        on through the `shared_decoder_tensors` slots (`_enqueue` skips the encoder, `_attach_grad` finds the graph).
        -> whether this call opened the slots itself (and has to close them)."""
        from . import train

        if not (isinstance(self.encoder, AttentionModelEncoder) and isinstance(self.decoder, AttentionModelDecoder)
                and hasattr(td, "items") and train.graph_encoder_equals_native(self, td)):
            if self.training and train.has_noisy_moe_encoder(self):
                # two encoder passes would draw two sets of gating noise: the rollout's log-likelihood and its gradient would
                # belong to differently routed networks
                raise NotImplementedError("training a noisy-gating MoE policy needs the single encoder pass, which serves the "
                                          "built-in AttentionModelEncoder / AttentionModelDecoder on fp32 GPU tensors only")
            return False
        own = getattr(self, "_shared_dt", None) is None
        if own:
            self._shared_dt = {}
        with torch.no_grad():
            ekey = train._graph_key(self, td)           # (the key `_enqueue` computes, under no_grad)
        ent = self._shared_dt.get("native")
        if ent is None or ent[0] != ekey:
            with torch.enable_grad():
                t = train.decoder_tensors(self, td)
            with torch.no_grad():
                init_embeds = self.encoder.init_embedding(td) if return_init_embeds else None
            self._shared_dt["native"] = (ekey, t["emb"].detach(), init_embeds, None)
        return own

    def _attach_grad(self, out: dict, p: dict) -> dict:
        from .train import evaluate_log_likelihood

        # select_best (decoding.py:419-427): `final_actions` are then the B best rows, re-evaluated as single rows whose first
        # column is the forced start node; top-k / top-p: the filtered entries are a fixed mask of the PyTorch re-evaluation
        best = p["S"] > 0 and p["select_best"]
        filtering = bool(p["top_k"]) or 0.0 < float(p["top_p"] or 0.0) < 1.0
        # the rollout's own per-step log-probs let the re-evaluation skip its forward pass (train.evaluate_log_likelihood)
        fl = p.get("final_logp")
        if fl is not None and (fl.shape != p["final_actions"].shape or os.environ.get("EAMRL_REEVAL_FORWARD", "0") == "1"
                               or filtering or best):
            fl = None
        fh = p.get("final_heads") if fl is not None else None       # (heads are only used together with the rollout's log-probs)
        # Given tours (actions=) with return_entropy: the entropy carries a graph too (PPO's entropy bonus, rl/ppo/ppo.py:168-209):
        # its value stays the one computed above, its gradient is the re-evaluation's.  A sampled rollout keeps the detached
        # entropy (the trainers only log it), and so does a filtered (top-k / top-p) or best-row re-evaluation.
        want_ent = bool(p.get("given_actions")) and p["return_entropy"] and "entropy" in out and not filtering and not best
        re = evaluate_log_likelihood(self, p["td"], p["env"], p["final_actions"], num_starts=0 if best else p["S"],
                                     multistart=bool(p["pre"]), temperature=p["temperature"],
                                     tanh_clipping=p["tanh_clipping"], rollout_logp=fl, rollout_heads=fh,
                                     top_k=int(p["top_k"] or 0), top_p=float(p["top_p"] or 0.0), return_entropy=want_ent)
        ent = None
        if want_ent:
            re, ent = re
            ent = ent.sum(1)
        td_mask = p["td"].get("mask", None) if hasattr(p["td"], "get") else None
        if td_mask is not None:
            re = re.masked_fill(~td_mask, 0)
        if p["return_sum_log_likelihood"]:
            re = re.sum(1)
        out = dict(out)
        out["log_likelihood"] = out["log_likelihood"].detach() + (re - re.detach())     # native value, re-eval gradient
        if ent is not None:
            out["entropy"] = out["entropy"].detach() + (ent - ent.detach())
        return out

    def _enqueue(self, td, env, phase, calc_reward, return_actions, return_entropy, return_hidden, return_init_embeds,
                 return_sum_log_likelihood, actions, max_steps, **decoding_kwargs) -> dict:
        if isinstance(env, str) or env is None:
            env = get_env(self.env_alias if env is None else env)
        if _kind(env.name) != self.env_name:
            raise ValueError(f"policy built for {self.env_alias!r} got env {env.name!r}")

        # decode type and strategy options (base.py:203-219, decoding.py:17-35,193-262)
        decode_type = decoding_kwargs.pop("decode_type", None)
        given_type = None
        if actions is not None:
            given_type, decode_type = decode_type, "evaluate"
        elif decode_type is None:
            decode_type = getattr(self, f"{phase}_decode_type")
        if decode_type == "beam_search":
            return {"out": self._beam_search(td, env, decoding_kwargs, calc_reward, return_actions,
                                             return_sum_log_likelihood, return_hidden, return_init_embeds, max_steps)}
        if decode_type not in DECODE_TYPES:
            log.warning("Unknown decode type '%s'. Defaulting to sampling.", decode_type)
            decode_type = "sampling"
        temperature = decoding_kwargs.pop("temperature", self.temperature)
        tanh_clipping = decoding_kwargs.pop("tanh_clipping", self.tanh_clipping)
        if not decoding_kwargs.pop("mask_logits", self.mask_logits):
            raise NotImplementedError("mask_logits=False is not built for MI355X")
        store_all_logp = decoding_kwargs.pop("store_all_logp", return_entropy)
        # The reference keeps every step's full log-prob vector only to compute the entropy from it (base.py:259-260) -- the
        # tensor itself is never returned.  Where the re-evaluation kernel covers the shape, the rollout stays one launch
        # and the entropy comes from one teacher-forced pass over the finished tours (`_native_entropy`) instead of a
        # host-driven step loop over [R, T, M] log-probs.
        entropy_native = False
        if store_all_logp and os.environ.get("EAMRL_ENTROPY_STEPWISE", "0") != "1":
            from .train import native_reeval_supported
            tk, tp = decoding_kwargs.get("top_k", 0) or 0, decoding_kwargs.get("top_p", 0.0) or 0.0
            Mq = td["action_mask"].shape[-1]
            if native_reeval_supported(self, Mq) and not tk and not (0.0 < tp < 1.0):
                store_all_logp, entropy_native = False, return_entropy
        num_starts = decoding_kwargs.pop("num_starts", None)
        num_samples = decoding_kwargs.pop("num_samples", None)
        multistart = decoding_kwargs.pop("multistart", False) or "multistart" in decode_type or (
            actions is not None and given_type is not None and "multistart" in given_type)
        multisample = decoding_kwargs.pop("multisample", False)
        select_best = decoding_kwargs.pop("select_best", False)
        select_start_nodes_fn = decoding_kwargs.pop("select_start_nodes_fn", None)
        decoding_kwargs.pop("softmax_temp", None)       # passed by SamplingEval; the reference's strategy ignores it too
        noise = decoding_kwargs.pop("noise", None)      # [R, T, M] Exp(1) draws replacing torch.multinomial's
        top_k = int(decoding_kwargs.pop("top_k", 0) or 0)          # process_logits filtering (decoding.py:170-176)
        top_p = float(decoding_kwargs.pop("top_p", 0.0) or 0.0)
        assert top_p <= 1.0, "top-p should be in (0, 1]."
        if decoding_kwargs:
            log.warning("ignored decoding kwargs: %s", list(decoding_kwargs))
        assert not (multistart and multisample), "Using both multistart and multisample is not supported"
        if num_samples is not None:
            multisample = num_samples > 1
        if num_starts is not None:
            multistart = num_starts > 1
        S = 0
        if multistart or multisample:
            S = num_starts if multistart else num_samples
            if S is None:
                S = env.get_num_starts(td)
        mode = "evaluate" if actions is not None else ("greedy" if "greedy" in decode_type else "sampling")

        # encoder + cache (one-shot); where the fused encoder kernel runs it also fills the cache from LDS
        spec = None
        if isinstance(self.encoder, AttentionModelEncoder) and isinstance(self.decoder, AttentionModelDecoder):
            Bq, Mq = td["action_mask"].shape
            spec = self.decoder._fused_cache_spec(Bq, Mq, td["action_mask"].device, dtype=self._dtype16)
        shared, ekey, ent = getattr(self, "_shared_dt", None), None, None
        # train.shared_decoder_tensors: same instances, same parameters (without a fused cache spec -- graphs above 128 nodes --
        # only for an MoE policy, to take over the embeddings of the training graph `_one_encoder_pass` has built: its gating
        # noise must be the rollout's)
        if shared is not None and (spec is not None or (shared.get("native") is not None and self._has_moe())):
            from .train import _graph_key

            ekey = _graph_key(self, td)
            ent = shared.get("native")
            ent = ent if ent is not None and ent[0] == ekey else None
        if ent is not None:
            hidden, init_embeds, spec = ent[1:]         # (spec None: embeddings of the training graph, cache GEMMs below)
            if init_embeds is None and return_init_embeds:
                init_embeds = self.encoder.init_embedding(td)
        else:
            if spec is not None and isinstance(self.encoder, AttentionModelEncoder):
                # the embeddings leave the kernel only when someone will read them (return_hidden, a second call sharing them)
                need_emb = (return_hidden or ekey is not None
                            or (self.decoder.use_graph_context and spec.get("gctx") is None))
                hidden, init_embeds = self.encoder(td, cache_spec=spec, want_hidden=need_emb, want_init=return_init_embeds)
            else:
                hidden, init_embeds = self.encoder(td, cache_spec=spec) if spec is not None else self.encoder(td)
            if ekey is not None and spec is not None and spec.get("filled"):
                shared["native"] = (ekey, hidden, init_embeds, spec)
        cache = self.decoder._precompute_cache(hidden, num_starts=S, prefilled=spec)

        # pre-decoder hook (decoding.py:284-332): multistart picks the first node, state replicated S times
        st = state_from_td(self.env_name, td, S)
        pre_actions, pre_logps = [], []
        if S >= 1 and multistart:
            if actions is not None:
                start, actions = actions[..., 0].contiguous(), actions[..., 1:]
            elif select_start_nodes_fn is not None:
                start = select_start_nodes_fn(td, env, S)
            else:
                start = env.select_start_nodes(td, num_starts=S)
            start = start.to(torch.int64).contiguous()
            _env_step_(st, start)
            pre_actions, pre_logps = [start[:, None]], [torch.zeros(st.R, 1, dtype=torch.float32, device=start.device)]

        # main decoding loop: one launch
        M = st.M
        t_max = _max_decode_steps(self.env_name, M, len(pre_actions))
        if self.env_name == "pdp" and not getattr(env, "force_start_at_depot", False):
            t_max -= 1              # every row takes exactly N steps: the arrays below carry no padding column
        t_max = int(max(1, min(t_max, max_steps)))
        given = None
        if actions is not None:
            given = actions.to(torch.int64).contiguous()
            t_max = min(t_max, given.shape[1]) if given.shape[1] > 0 else t_max
        seed = seed_dev = None
        if mode == "sampling":
            if noise is None and not store_all_logp:
                # no noise tensor: the draws are a function of (seed, row, step, node), computed inside the rollout kernel
                # where it can (ops.rollout).  Eagerly the seed comes from torch's CPU generator (torch.manual_seed
                # reproduces it); under HIP-graph capture it is a device word refilled by a captured random_() per replay.
                if torch.cuda.is_current_stream_capturing():
                    seed = 0
                    seed_dev = torch.empty(1, dtype=torch.int64, device=st.mask.device).random_()
                else:
                    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
                    # data-parallel replicas are usually seeded alike (and the noise is a pure function of (seed, row, step,
                    # node)): mix the rank in so that the ranks explore with independent noise fields
                    if torch.distributed.is_available() and torch.distributed.is_initialized():
                        seed ^= (torch.distributed.get_rank() * 0x9E3779B97F4A7C15) & (2 ** 62 - 1)
            elif noise is None:
                noise = torch.empty(st.R, t_max, M, dtype=torch.float32, device=st.mask.device).exponential_(1)
            else:
                noise = noise.to(device=st.mask.device, dtype=torch.float32)
                if noise.dim() != 3 or noise.shape[0] != st.R or noise.shape[2] != M:
                    raise ValueError(f"noise must be [R={st.R}, T, M={M}], got {tuple(noise.shape)}")
                t_max = min(t_max, noise.shape[1])        # a shorter noise tensor bounds the episode length
                noise = noise[:, :t_max].contiguous()     # the kernel strides rows by t_max * M
        all_logp = None
        dev = st.mask.device
        if store_all_logp:
            acts, lps, all_logp, T, status = self._rollout_stepwise(st, cache, mode, noise, given, tanh_clipping,
                                                                    temperature, t_max, top_k, top_p)
            info = None
        else:
            # training (multistart): the start-sharing kernel also keeps every step's glimpse output for the backward
            acts, lps, info = ops.rollout(st, cache, mode, noise=noise, given=given, clip=tanh_clipping,
                                          temp=temperature, t_max=t_max, top_k=top_k, top_p=top_p, seed=seed, seed_dev=seed_dev,
                                          return_flags=True,          # int32[4]: steps, status, 2 free validity counters
                                          poly=self._pointer_operands(),
                                          want_heads=bool(getattr(self, "_want_heads", False)) and bool(pre_actions))
        # Everything below is enqueued on the PADDED [R, t_max] arrays before the rollout's single host sync:
        # padding is depot visits with log-prob 0, which change neither the tour length (zero-length legs, and
        # x + 0 is exact in the lane tree), nor the log-likelihood sum, nor validity.
        actions_pad = torch.cat(pre_actions + [acts], 1) if pre_actions else acts
        logp_pad = torch.cat(pre_logps + [lps], 1) if pre_logps else lps
        native_env = type(env) in ENV_REGISTRY.values()
        fast = info is not None and native_env and not select_best
        reward_pad = ll_pad = bad = None
        one_launch = fast and self.env_name in ("tsp", "cvrp") and calc_reward
        if one_launch:              # reward + validity + log-likelihood of a row by one wavefront, one launch
            want_ll = return_sum_log_likelihood and "mask" not in td.keys()
            bad = info[2:] if env.check_solution else None
            reward_pad, ll_pad = ops.rollout_finish(self.env_name, td["locs"].contiguous(), actions_pad,
                                                    logp_pad if want_ll else None,
                                                    td["demand"].contiguous() if self.env_name == "cvrp" else None,
                                                    st.vcap, bad=bad)
        elif fast:
            # a one-step episode (max_steps = 1, or one given column) of PCTSP / OP is the reference's "length 1 tours"
            # special case, which lives in the env classes: `_finish` then asks env.get_reward on the exact slice
            if calc_reward and not (actions_pad.shape[1] == 1 and self.env_name in ("pctsp", "op")):
                spec = ENV_SPECS[self.env_name]
                reward_pad = ops.call_spec(spec.reward, td, actions_pad)
                if env.check_solution and spec.check_padded != "no":        # "no": checked in _finish, on the exact slice
                    bad = ops.call_spec(spec.check, td, actions_pad, st.vcap)
            if return_sum_log_likelihood and "mask" not in td.keys():
                ll_pad = ops.sum_logp(logp_pad)
        flags = None
        if info is not None:
            if one_launch:
                flags = info if bad is not None else info[:2]
            else:
                flags = torch.cat((info[:2], bad)) if bad is not None else info[:2]
        else:
            flags = torch.tensor([T, status], dtype=torch.int32)
        return dict(flags=flags, has_bad=bad is not None, pre=1 if pre_actions else 0, t_max=t_max, M=M, S=S,
                    temperature=temperature, tanh_clipping=tanh_clipping, top_k=top_k, top_p=top_p,
                    select_best=select_best, calc_reward=calc_reward, env=env, st=st, td=td, cache=cache,
                    actions_pad=actions_pad, logp_pad=logp_pad, reward_pad=reward_pad, ll_pad=ll_pad,
                    all_logp=all_logp, entropy_native=entropy_native, init_embeds=init_embeds, return_actions=return_actions,
                    return_entropy=return_entropy, return_hidden=return_hidden, return_init_embeds=return_init_embeds,
                    return_sum_log_likelihood=return_sum_log_likelihood, final_heads=getattr(st, "heads", None))

    def _finish(self, p: dict) -> dict:
        vals = p["flags"].tolist()               # the rollout's single device->host sync
        T, status = vals[0], vals[1]
        bad_counts = vals[2:] if p["has_bad"] else None
        env, st, td, S, M = p["env"], p["st"], p["td"], p["S"], p["M"]
        ops.raise_on_status(status)
        if status & ops.ST_STEP_OVERRUN:
            log.error("Exceeded maximum number of steps (%d) during decoding", p["t_max"])
        npre = p["pre"]
        assert T > 0 or npre, \
            "No logprobs were collected because all environments were done. Check your initial state"
        actions_out = p["actions_pad"][:, :npre + T]
        logprobs = p["logp_pad"][:, :npre + T]
        td_out = state_to_td(self.env_name, st, td)
        if self.env_name == "pdp" and "i" in td_out.keys():
            td_out.set("i", td_out["i"] + (npre + T))

        if S > 0 and p["select_best"]:   # DecodingStrategy._select_best (decoding.py:419-427)
            rewards = env.get_reward(td_out, actions_out)
            _, max_idxs = unbatchify(rewards, S).max(dim=-1)
            actions_out = unbatchify_and_gather(actions_out, max_idxs, S)
            logprobs = unbatchify_and_gather(logprobs, max_idxs, S)
            td_out = TensorDict({k: unbatchify_and_gather(v, max_idxs, S) for k, v in td_out.items()},
                                batch_size=[max_idxs.shape[0]])

        if p["calc_reward"]:
            if p["reward_pad"] is not None:
                spec = ENV_SPECS[self.env_name]
                # if_full (TSP): node 0 is a real city, so zero padding can be neither checked nor measured in place:
                # the (rare) short episode is re-checked and its reward recomputed on the exact slice
                short = spec.check_padded == "if_full" and npre + T != p["actions_pad"].shape[1]
                if bad_counts is not None and not short:
                    assert bad_counts[0] == 0, spec.messages[0]
                    assert bad_counts[1] == 0, spec.messages[1]
                elif env.check_solution and (short or spec.check_padded == "no"):
                    env.check_solution_validity(td_out, actions_out.contiguous())
                if short:
                    td_out.set("reward", env.get_reward(td_out, actions_out.contiguous(), check_solution=False))
                else:
                    td_out.set("reward", p["reward_pad"])
            else:
                td_out.set("reward", env.get_reward(td_out, actions_out.contiguous()))
        td_mask = td_out.get("mask", None)
        if td_mask is not None:
            logprobs = logprobs.masked_fill(~td_mask, 0)
        # get_log_likelihood (decoding.py:38-64); -inf would mean an infeasible action slipped through
        if p["return_sum_log_likelihood"]:
            ll = p["ll_pad"] if p["ll_pad"] is not None else ops.sum_logp(logprobs)
        else:
            ll = logprobs
        out = {"reward": td_out["reward"], "log_likelihood": ll}
        if p["return_actions"]:
            out["actions"] = actions_out
        if p["return_entropy"]:
            if p.get("entropy_native"):
                out["entropy"] = self._native_entropy(p, actions_out)
            else:
                lp = torch.nan_to_num(p["all_logp"], nan=0.0, neginf=0.0)
                out["entropy"] = -(lp.exp() * lp).sum(-1).sum(1)
        if p["return_hidden"]:
            out["hidden"] = p["cache"]
        if p["return_init_embeds"]:
            out["init_embeds"] = p["init_embeds"]
        self._last_td = td_out   # final env state of the last rollout (the reference keeps it in a local)
        p["final_actions"] = actions_out
        p["final_logp"] = logprobs if not (S > 0 and p["select_best"]) else None
        return out

    @torch.no_grad()
    def _native_entropy(self, p: dict, actions_out: torch.Tensor) -> torch.Tensor:
        """calculate_entropy (rl4co/utils/ops.py: -(p log p) summed over nodes and steps) of the finished tours [R, T]: one
        launch of the teacher-forced forward kernel on the decoder cache of this very rollout, the env states replayed from
        the actions (train.replay_states).  Forced steps (the multistart column, rows that are done) contribute 0, as the
        reference's one-hot log-prob vectors do.  Hardware exp / log: within 1e-5 of the step-wise computation."""
        from .train import replay_states

        cache = p["cache"]
        if p["S"] > 0 and p["select_best"]:
            raise NotImplementedError("return_entropy together with select_best")
        acts = actions_out.contiguous()
        S = max(int(p["S"]), 1)
        meta = replay_states(self, p["td"], acts, S, bool(p["pre"]))
        E = cache.E
        if self.env_name == "tsp":
            cvec = cache.cvec.reshape(1, E).contiguous() if meta["placeholder"] else None
        else:
            cvec = cache.cvec.reshape(-1, E).contiguous()
        slots = {n: cache.slots[n] for n in ("K", "V", "Lp", "Pa") + (("Pb",) if "Pb" in cache.slots else ())}
        plan = ops.ReevalPlan(cache.buf, "Pb" in cache.slots, cache.gctx, cvec, meta["idxA"], meta["idxB"], meta["sc"],
                              meta["maskbits"], acts, S, meta["tstart"], float(p["tanh_clipping"]), float(p["temperature"]),
                              slots=slots, E=E, want_entropy=True, rollout_heads=p.get("final_heads"),
                              rem=meta.get("rem"), dyn=cache.dyn if meta.get("rem") is not None else None)     # (SDVRP)
        plan.forward()
        return plan.entropy.sum(1)

    def _beam_search(self, td, env, kw, calc_reward, return_actions, return_sum_log_likelihood, return_hidden,
                     return_init_embeds, max_steps):
        """decode_type="beam_search" (BeamSearch, rl4co/utils/decoding.py:468-608): the beams start from the
        multistart nodes; every step keeps, per instance, the beam_width best (beam, node) continuations by cumulative
        log-prob (`eamrl_beam_topk`), and each new beam inherits the state of its parent.  Host-driven step loop on
        the step API, as the reference's; afterwards the tours are backtracked through the parent pointers."""
        beam_width = kw.pop("beam_width", None)
        select_best = kw.pop("select_best", True)
        temperature = kw.pop("temperature", self.temperature)
        tanh_clipping = kw.pop("tanh_clipping", self.tanh_clipping)
        select_start_nodes_fn = kw.pop("select_start_nodes_fn", None)
        top_k, top_p = int(kw.pop("top_k", 0) or 0), float(kw.pop("top_p", 0.0) or 0.0)
        for k in ("store_all_logp", "num_starts", "multistart"):
            kw.pop(k, None)
        if kw:
            log.warning("ignored decoding kwargs: %s", list(kw))
        BW = env.get_num_starts(td) if beam_width is None else int(beam_width)
        assert BW > 1, "beam width must be larger than 1"
        hidden, init_embeds = self.encoder(td)
        cache = self.decoder._precompute_cache(hidden, num_starts=BW)
        B = td.batch_size[0]
        st = state_from_td(self.env_name, td, BW)
        start = (select_start_nodes_fn(td, env, BW) if select_start_nodes_fn is not None
                 else env.select_start_nodes(td, num_starts=BW)).to(torch.int64).contiguous()
        _env_step_(st, start)
        dev = start.device
        R, M = st.R, st.M
        inst = torch.arange(B, device=dev).repeat(BW)
        actions, step_lps = [start], [torch.zeros(R, dtype=torch.float32, device=dev)]
        parents = [torch.zeros(R, dtype=torch.int64, device=dev)]
        parent_lp = torch.zeros(R, dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        t_max = int(max(1, min(_max_decode_steps(self.env_name, M, 1), max_steps)))
        t = 0
        while t < t_max and not bool(st.done.all()):
            _, _, all_lp, _, _ = ops.decode_step(st, cache, "greedy", clip=tanh_clipping, temp=temperature,
                                                 fuse_env_step=False, want_logprobs=True, status=status,
                                                 top_k=top_k, top_p=top_p)
            node, beam, parent_lp, slp = ops.beam_topk(all_lp, parent_lp, B, BW)
            beam = beam.to(torch.int64)
            st.reorder_(inst + beam * B)
            _env_step_(st, node)
            actions.append(node)
            step_lps.append(slp)
            parents.append(beam)
            t += 1
        ops.raise_on_status(int(status.item()))
        if t == t_max and not bool(st.done.all()):
            log.error("Exceeded maximum number of steps (%d) during decoding", t_max)
        # backtrack (BeamSearch._backtrack): walk the parent pointers from the last step to the first
        acts = torch.stack(actions, 1)
        lps = torch.stack(step_lps, 1)
        T = acts.shape[1]
        cur_parent = parents[-1]
        seq, seq_lp = [acts[:, -1]], [lps[:, -1]]
        for k in range(T - 2, -1, -1):
            idx = inst + cur_parent * B
            seq.append(acts[idx, k])
            seq_lp.append(lps[idx, k])
            cur_parent = parents[k][idx]
        actions_out = torch.stack(seq[::-1], 1).contiguous()
        logprobs = torch.stack(seq_lp[::-1], 1).contiguous()
        td_out = state_to_td(self.env_name, st, td)
        if select_best:     # BeamSearch._select_best_beam
            rewards = env.get_reward(td_out, actions_out)
            best = unbatchify(rewards, BW).max(dim=-1).indices
            flat = torch.arange(B, device=dev) + best * B
            actions_out, logprobs = actions_out[flat].contiguous(), logprobs[flat].contiguous()
            td_out = TensorDict({k: v[flat] for k, v in td_out.items()}, batch_size=[B])
        if calc_reward:
            td_out.set("reward", env.get_reward(td_out, actions_out))
        out = {"reward": td_out["reward"],
               "log_likelihood": ops.sum_logp(logprobs) if return_sum_log_likelihood else logprobs}
        if return_actions:
            out["actions"] = actions_out
        if return_hidden:
            out["hidden"] = cache
        if return_init_embeds:
            out["init_embeds"] = init_embeds
        self._last_td = td_out
        return out

    def _rollout_stepwise(self, st, cache, mode, noise, given, clip, temp, t_max, top_k=0, top_p=0.0):
        """Step-API loop (one fused decode+env launch per step) used when every step's full log-prob row
        is wanted (store_all_logp / return_entropy).  The loop condition is checked on the host each step,
        as the reference does."""
        acts, lps, alls = [], [], []
        status = torch.zeros(1, dtype=torch.int32, device=st.mask.device)
        t = 0
        while t < t_max and not bool(st.done.all()):
            a, lp, all_lp, _, _ = ops.decode_step(
                st, cache, mode, noise=None if noise is None else noise[:, t].contiguous(),
                given=None if given is None else given[:, t].contiguous(), clip=clip, temp=temp,
                fuse_env_step=True, want_logprobs=True, status=status, top_k=top_k, top_p=top_p)
            acts.append(a)
            lps.append(lp)
            alls.append(all_lp)
            t += 1
        R, M = st.R, st.M
        dev = st.mask.device
        acts = torch.stack(acts, 1) if acts else torch.zeros(R, 0, dtype=torch.int64, device=dev)
        lps = torch.stack(lps, 1) if lps else torch.zeros(R, 0, dtype=torch.float32, device=dev)
        alls = torch.stack(alls, 1) if alls else torch.zeros(R, 0, M, dtype=torch.float32, device=dev)
        return acts, lps, alls, t, int(status.item())


class HeterogeneousAttentionModelPolicy(AttentionModelPolicy):
    """Heterogeneous Attention Model (Li et al. 2021) for pickup and delivery: Kool's model with the encoder whose attention
    also scores a node's partner, the nodes of its own role and those of the other role (zoo/ham/policy.py:9-62, same
    constructor arguments).  Decoder, context, cache, env and reward are AttentionModelPolicy's for PDP."""

    def __init__(self, encoder: nn.Module = None, env_name: str = "pdp", init_embedding: nn.Module = None, embed_dim: int = 128,
                 num_encoder_layers: int = 3, num_heads: int = 8, normalization: str = "batch", feedforward_hidden: int = 512,
                 sdpa_fn=None, **kwargs):
        if encoder is None:
            encoder = GraphHeterogeneousAttentionEncoder(init_embedding=init_embedding, num_heads=num_heads, embed_dim=embed_dim,
                                                         num_encoder_layers=num_encoder_layers, env_name=env_name,
                                                         normalization=normalization, feedforward_hidden=feedforward_hidden,
                                                         sdpa_fn=sdpa_fn)
        super().__init__(env_name=env_name, encoder=encoder, embed_dim=embed_dim, num_encoder_layers=num_encoder_layers,
                         num_heads=num_heads, normalization=normalization, **kwargs)


class PolyNetDecoder(AttentionModelDecoder):
    """AttentionModelDecoder with the PolyNet pointer (zoo/polynet/decoder.py:27-112, same arguments and state-dict keys).
    Cache, context and dynamic embedding are the Attention Model's; the pointer's extra operands go to the rollout kernel
    through `poly_operands`."""

    is_polynet = True

    def __init__(self, k: int, encoder_type: str = "AM", embed_dim: int = 128, poly_layer_dim: int = 256, num_heads: int = 8,
                 env_name="tsp", context_embedding=None, dynamic_embedding=None, mask_inner: bool = True,
                 out_bias_pointer_attn: bool = False, linear_bias: bool = False, use_graph_context: bool = True,
                 check_nan: bool = True, sdpa_fn=None, **unused_kwargs):
        from .attention import PolyNetAttention

        if encoder_type != "AM":
            raise NotImplementedError(f"PolyNetDecoder: encoder_type={encoder_type!r} is not built for MI355X (the MatNet encoder "
                                      "and its row / column cache are not part of this library); use encoder_type='AM'")
        if poly_layer_dim != ops.POLY_LAYER_DIM:
            raise NotImplementedError(f"PolyNetDecoder: poly_layer_dim={poly_layer_dim}; the rollout kernel is built for "
                                      f"{ops.POLY_LAYER_DIM} (the reference's default)")
        if isinstance(env_name, RL4COEnvBase):
            env_name = env_name.name
        if _kind(env_name) not in ("tsp", "cvrp"):
            raise NotImplementedError(f"PolyNetDecoder: env_name={env_name!r}; the PolyNet rollout kernel is built for 'tsp' and "
                                      "'cvrp' (SDVRP's dynamic embedding, PDP and the other envs are not)")
        if embed_dim != 128 or num_heads != 8:
            raise NotImplementedError("PolyNetDecoder: the rollout kernel is built for embed_dim=128, num_heads=8")
        pointer = PolyNetAttention(k, embed_dim, poly_layer_dim, num_heads, mask_inner=mask_inner, out_bias=out_bias_pointer_attn,
                                   check_nan=check_nan, sdpa_fn="default" if sdpa_fn is None else sdpa_fn)
        super().__init__(embed_dim=embed_dim, num_heads=num_heads, env_name=env_name, context_embedding=context_embedding,
                         dynamic_embedding=dynamic_embedding, mask_inner=mask_inner, out_bias_pointer_attn=out_bias_pointer_attn,
                         linear_bias=linear_bias, use_graph_context=use_graph_context, check_nan=check_nan, pointer=pointer)
        self.encoder_type, self.k = encoder_type, k

    def poly_operands(self):
        """ops.polynet_operands of the pointer's parameters, recomputed when one of them changes (optimizer step, load) and
        refreshed in place where the shapes allow, like `_weight_constants`."""
        ptr = self.pointer
        srcs = (ptr.project_out.weight, ptr.poly_layer_1.weight, ptr.poly_layer_1.bias, ptr.poly_layer_2.weight,
                ptr.poly_layer_2.bias, ptr.binary_vectors)
        key = tuple((t.data_ptr(), t._version) for t in srcs)
        if getattr(self, "_poly_key", None) != key:
            new = ops.polynet_operands(*srcs)
            old = self.__dict__.get("_poly")
            if old is not None and all(isinstance(v, int) or (v.shape == old[n].shape and v.device == old[n].device)
                                       for n, v in new.items()):
                for n, v in new.items():
                    if isinstance(v, int):
                        old[n] = v
                    else:
                        old[n].copy_(v)
            else:
                self.__dict__["_poly"] = new
            self._poly_key = key
        return self.__dict__["_poly"]

    def forward(self, td, cached, num_starts: int = 0):
        raise NotImplementedError("PolyNetDecoder: a single decode step is not built for MI355X; PolyNetPolicy rolls out in one "
                                  "launch per 128 solutions of an instance")


class PolyNetPolicy(AttentionModelPolicy):
    """PolyNet (Hottung et al. 2024; zoo/polynet/policy.py:10-99, same arguments and defaults): the Attention Model encoder
    (POMO's settings) with the PolyNet decoder, k strategies per instance.  Rollouts are multi-row per instance --
    `policy(td, env, num_starts=S, multisample=True)` as PolyNet.shared_step calls it (zoo/polynet/model.py:141-148) -- and run
    in the PolyNet case of the start-sharing kernel; everything else raises NotImplementedError (there is no PyTorch rollout)."""

    def __init__(self, k: int, encoder: nn.Module = None, encoder_type: str = "AM", embed_dim: int = 128,
                 num_encoder_layers: int = 6, num_heads: int = 8, normalization: str = "instance",
                 feedforward_hidden: int = 512, env_name="tsp", temperature: float = 1.0, tanh_clipping: float = 10.0,
                 mask_logits: bool = True, train_decode_type: str = "sampling", val_decode_type: str = "sampling",
                 test_decode_type: str = "sampling", **kwargs):
        if encoder_type != "AM":
            raise NotImplementedError(f"PolyNetPolicy: encoder_type={encoder_type!r} is not built for MI355X (no MatNet encoder in "
                                      "this library); use encoder_type='AM'")
        dec_kw = {n: kwargs.pop(n) for n in ("poly_layer_dim", "use_graph_context", "check_nan", "mask_inner",
                                             "out_bias_pointer_attn") if n in kwargs}
        if isinstance(env_name, RL4COEnvBase):
            env_name = env_name.name
        decoder = PolyNetDecoder(k=k, encoder_type=encoder_type, embed_dim=embed_dim, num_heads=num_heads, env_name=env_name,
                                 **dec_kw)
        super().__init__(encoder=encoder, decoder=decoder, embed_dim=embed_dim, num_encoder_layers=num_encoder_layers,
                         num_heads=num_heads, normalization=normalization, feedforward_hidden=feedforward_hidden,
                         env_name=env_name, temperature=temperature, tanh_clipping=tanh_clipping, mask_logits=mask_logits,
                         train_decode_type=train_decode_type, val_decode_type=val_decode_type,
                         test_decode_type=test_decode_type, **kwargs)
        self.k = k

    def _pointer_operands(self):
        return self.decoder.poly_operands()

    def _enqueue(self, td, env, phase, calc_reward, return_actions, return_entropy, return_hidden, return_init_embeds,
                 return_sum_log_likelihood, actions, max_steps, **decoding_kwargs):
        kw = decoding_kwargs
        decode_type = kw.get("decode_type") or getattr(self, f"{phase}_decode_type")
        if decode_type == "beam_search":
            raise NotImplementedError("PolyNetPolicy: beam search is not built (its step loop runs the per-step decoder)")
        if return_entropy or kw.get("store_all_logp"):
            raise NotImplementedError("PolyNetPolicy: return_entropy / store_all_logp are not built (they need the per-step "
                                      "decoder or the re-evaluation kernel, neither has the PolyNet layers)")
        if kw.get("top_k") or 0.0 < float(kw.get("top_p") or 0.0) < 1.0:
            raise NotImplementedError("PolyNetPolicy: top-k / top-p filtering is not built into the PolyNet rollout kernel")
        if kw.get("select_best"):
            raise NotImplementedError("PolyNetPolicy: select_best is not built; take the best of out['reward'] per instance")
        S = kw.get("num_starts") if kw.get("num_starts") is not None else kw.get("num_samples")
        many = (S is not None and S > 1) or (S is None and (kw.get("multistart") or kw.get("multisample")
                                                            or "multistart" in decode_type))
        if not many:
            raise NotImplementedError("PolyNetPolicy: rollouts with one row per instance are not built; PolyNet decodes several "
                                      "solutions per instance: policy(td, env, num_starts=S, multisample=True) with S >= 2")
        if td["action_mask"].shape[-1] > 112:
            raise NotImplementedError(f"PolyNetPolicy: graphs above 112 nodes are not built (got {td['action_mask'].shape[-1]})")
        return super()._enqueue(td, env, phase, calc_reward, return_actions, return_entropy, return_hidden, return_init_embeds,
                                return_sum_log_likelihood, actions, max_steps, **decoding_kwargs)


def load_reference_checkpoint(policy: AttentionModelPolicy, ckpt, strict: bool = True):
    """Load the policy weights of a reference Lightning checkpoint.

    `ckpt` is a path (read with torch.load(weights_only=True): nothing from the file is executed), a Lightning
    checkpoint dict (`{"state_dict": {...}}`) or a plain state_dict.  Keys of the LitModule carry the prefix
    `policy.` (rl4co/models/rl/common/base.py); `baseline.*` entries (rollout-baseline copy of the policy,
    reinforce.py:198-210) and anything else outside the policy are ignored."""
    if isinstance(ckpt, (str, bytes)) or hasattr(ckpt, "__fspath__"):
        ckpt = torch.load(ckpt, map_location="cpu", weights_only=True)
    sd = ckpt.get("state_dict", ckpt) if isinstance(ckpt, dict) else ckpt
    has_prefix = any(k.startswith("policy.") for k in sd)
    own = {}
    for k, v in sd.items():
        if has_prefix:
            if not k.startswith("policy."):
                continue
            k = k[len("policy."):]
        elif k.startswith("baseline."):
            continue
        own[k] = v
    return policy.load_state_dict(own, strict=strict)


def rollout(env, td, policy, max_steps: int = None):
    """Test helper with the reference's signature (utils/decoding.py:87-108): policy is a callable td -> td
    that sets td["action"]."""
    max_steps = float("inf") if max_steps is None else max_steps
    actions, steps = [], 0
    while not td["done"].all():
        td = policy(td)
        actions.append(td["action"])
        td = env.step(td)["next"]
        steps += 1
        if steps > max_steps:
            break
    actions = torch.stack(actions, 1)
    return env.get_reward(td, actions), td, actions


def random_policy(td):
    """Uniform choice among feasible actions (utils/decoding.py:80-84)."""
    td.set("action", torch.multinomial(td["action_mask"].float(), 1).squeeze(-1))
    return td


class SymNCOPolicy(AttentionModelPolicy):
    """AttentionModelPolicy + the projection head of SymNCO (rl4co/models/zoo/symnco/policy.py:13-96): `forward` also returns
    `proj_embeddings = projection_head(init_embeds)`, which the invariance loss of SymNCO / SymEAM compares across the
    augmented copies of an instance (zoo/symnco/losses.py:31-39, zoo/earl/model.py:471-712).  The head is torchrl's
    `MLP(E, E, depth 1, E, ReLU)` = Linear, ReLU, Linear with state_dict keys `projection_head.{0,2}.{weight,bias}`.

    Under autograd (phase "train") the init embeddings handed to the head are the differentiable ones (the tiny-K Linear of
    the training graph, train._small_linear -- same values as the rollout's, bit for bit), so the invariance loss reaches
    the init-embedding weights as it does in the reference."""

    def __init__(self, embed_dim: int = 128, env_name: str = "tsp", num_encoder_layers: int = 3, num_heads: int = 8,
                 normalization: str = "batch", projection_head: nn.Module = None, use_projection_head: bool = True, **kwargs):
        super().__init__(env_name=env_name, embed_dim=embed_dim, num_encoder_layers=num_encoder_layers, num_heads=num_heads,
                         normalization=normalization, **kwargs)
        self.use_projection_head = use_projection_head
        if use_projection_head:
            self.projection_head = projection_head if projection_head is not None else nn.Sequential(
                nn.Linear(embed_dim, embed_dim), nn.ReLU(), nn.Linear(embed_dim, embed_dim))

    def forward(self, td, env=None, phase: str = "train", return_actions: bool = True, return_init_embeds: bool = True, **kwargs):
        assert not (self.use_projection_head and not return_init_embeds), \
            "If `use_projection_head` is True, then we must `return_init_embeds`"
        out = super().forward(td, env, phase, return_actions=return_actions, return_init_embeds=return_init_embeds, **kwargs)
        if self.use_projection_head:
            init = out["init_embeds"]
            if torch.is_grad_enabled() and phase == "train" and not torch.is_inference_mode_enabled():
                from .train import init_embedding_autograd

                init = init_embedding_autograd(self, td)
                out = dict(out)
                out["init_embeds"] = init
            head = self.projection_head
            if isinstance(head, nn.Sequential) and len(head) == 3 and isinstance(head[0], nn.Linear) and isinstance(head[2], nn.Linear):
                from .train import _linear

                out["proj_embeddings"] = _linear(_linear(init, head[0].weight, head[0].bias, relu=True), head[2].weight, head[2].bias)
            else:
                out["proj_embeddings"] = head(init)
        return out


class GraphedRollout:
    """`policy(td, env, **kwargs)` for a fixed batch shape, captured once into a HIP graph and replayed.

    A rollout is ~45 short launches (encoder GEMMs, attention, cache, the decode loop, reward); replaying them as
    one graph removes the per-launch host cost, which dominates small problems (TSP-20) and is ~8 % at TSP-100
    B=1024.  Only the device half of `forward` (`_enqueue`) is captured; the single host sync and the output
    slicing (`_finish`) run after every replay.  Outputs are copies, so they stay valid across replays.
    Not capturable: return_entropy / store_all_logp (host-driven step loop) and select_best.
    """

    def __init__(self, policy: AttentionModelPolicy, env: RL4COEnvBase, td_example, warmup: int = 2, phase="test",
                 **forward_kwargs):
        if (forward_kwargs.get("return_entropy") or forward_kwargs.get("store_all_logp") or forward_kwargs.get("select_best")
                or forward_kwargs.get("decode_type") == "beam_search"):
            raise NotImplementedError("GraphedRollout: step-wise / select_best / beam-search rollouts are not capturable")
        if isinstance(policy, PolyNetPolicy):
            raise NotImplementedError("GraphedRollout: capture of a PolyNet rollout has not been built or tested")
        if getattr(policy, "is_ptrnet", False):
            raise NotImplementedError("GraphedRollout: capture of a Pointer Network rollout has not been built or tested")
        self.policy, self.env = policy, env
        self.kw = dict(phase=phase, calc_reward=True, return_actions=True, return_entropy=False, return_hidden=False,
                       return_init_embeds=False, return_sum_log_likelihood=True, actions=None, max_steps=1_000_000)
        self.kw.update(forward_kwargs)
        self.static_td = td_example.clone()
        self._training = policy.training
        self._precision = policy.precision
        M = td_example["action_mask"].shape[1]
        self._embed_probe = torch.empty(1, M, policy.decoder.embed_dim, device=td_example["action_mask"].device)
        self._keys = [k for k, v in self.static_td.items() if isinstance(v, torch.Tensor)]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(max(1, warmup)):      # sets kernel attributes, fills caches, warms the allocator
                policy._finish(policy._enqueue(self.static_td, env, **self.kw))
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self._pending = policy._enqueue(self.static_td, env, **self.kw)     # works on copies of the state tensors
        self._tensors = list(policy.parameters()) + list(policy.buffers())
        self._sig = None                                                        # first call: look at everything

    def _weights_signature(self):
        """(sum of in-place version counters, sum of storage addresses) over parameters and buffers: changes with every
        optimizer step / load_state_dict / replaced tensor."""
        v = a = 0
        for t in self._tensors:
            v += t._version
            a += t.data_ptr()
        return v, a

    @torch.no_grad()
    def __call__(self, td) -> dict:
        if self.policy.training != self._training:
            raise RuntimeError("GraphedRollout: policy.train() / .eval() changed since capture (different launches)")
        if self.policy.precision != self._precision:
            raise RuntimeError(f"GraphedRollout: policy.precision changed since capture ({self._precision!r} -> "
                               f"{self.policy.precision!r}: different kernels)")
        # weight-derived constants live in persistent buffers that the graph reads: refresh them in place when a
        # parameter changed (optimizer step, load_state_dict); everything else the graph reads are the live parameters.
        # One pass over the version counters decides whether anything has to be looked at.
        sig = self._weights_signature()
        if sig != self._sig:
            self._sig = sig
            self.policy.decoder._weight_constants()
            dec, dtype = self.policy.decoder, self.policy._dtype16
            if hasattr(dec, "_fused_cache_spec") and (getattr(dec, "_fc", None) if dtype is None
                                                      else getattr(dec, "_fc16", {}).get(dtype)) is not None:
                M = self._embed_probe.shape[1]
                dec._fused_cache_spec(0, M, self._embed_probe.device, dtype=dtype)    # re-packs in place when weights changed
            net = getattr(self.policy.encoder, "net", None)
            if hasattr(net, "_fused_layers"):
                net._fused_layers(self._embed_probe)          # re-packs changed encoder weights into the buffers the graph reads
            for layer in getattr(net, "layers", ()):
                ffn = getattr(layer[2], "module", None) if isinstance(layer, nn.Sequential) and len(layer) > 2 else None
                if isinstance(ffn, MoE):
                    ffn.packed_experts()                      # ... and the MoE layers' expert packs
            refresh = getattr(self.policy.encoder, "refresh_packs", None)
            if refresh is not None:
                refresh()
        pairs = []
        for k in self._keys:
            src = td[k]
            dst = self.static_td[k]
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError(f"GraphedRollout was captured for {k}: {tuple(dst.shape)} {dst.dtype}")
            if src.is_contiguous() and dst.is_contiguous() and src.device == dst.device:
                pairs.append((dst, src))
            else:
                dst.copy_(src)
        if pairs:
            ops.multi_copy_(pairs)       # all inputs in one launch
        self.graph.replay()
        out = self.policy._finish(self._pending)
        return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
