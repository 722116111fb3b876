"""Training companion of the native rollout: gradients by teacher-forced re-evaluation.

The rollout itself runs on the HIP kernels without a graph.  For REINFORCE / POMO / EAM the log-likelihood of the
*chosen* actions is what must be differentiated; because the actions are known after the rollout, every decode
step's state (current / first node, visited set, used capacity) is a prefix function of the action sequence, so all
T steps are re-evaluated AT ONCE as dense batched contractions -- the same trick serves EAM's
`policy(..., actions=improved)` pass (rl4co/models/zoo/earl/model.py:179-195).
`AttentionModelPolicy.forward(phase="train")` attaches this re-evaluation to the `log_likelihood` it returns
(`attach_log_likelihood_grad`): the value is the native rollout's, the gradient is the re-evaluation's, so the
reference's trainers (`out["log_likelihood"]` -> loss -> backward, reinforce.py:79-106, pomo/model.py:89-112) run on
the policy unchanged.  This module is the gradient path only: it is not used by inference, benchmarks or parity tests
of the rollout, and its forward values are checked against the native log-probs (tests/test_gpu_next.py,
tests/test_gpu_train.py).

Reference call sites: rl4co/models/rl/reinforce/reinforce.py:59-106 (REINFORCE.shared_step / calculate_loss),
rl4co/models/rl/reinforce/baselines.py:57-61 (SharedBaseline), rl4co/models/zoo/pomo/model.py:89-148.
"""
from __future__ import annotations

import os

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .env_spec import ENV_SPECS
from .utils import unbatchify


# ------------------------------------------------------------------------------------------------------------
# differentiable encoder + cache (same parameters as the native path)
# ------------------------------------------------------------------------------------------------------------
class _InstanceNormFn(torch.autograd.Function):
    """InstanceNorm1d(affine) on [B, N, E] as it lies (eamrl_instance_norm_forward / _backward): torch's instance_norm needs
    [B, E, N] -- two transposed copies per call -- and runs MIOpen's spatial batch-norm kernels (0.49 ms per backward at
    1024 x 100 x 128; the POMO encoder has 12 of them)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        from . import ops

        xc = x.contiguous()
        y, mean, rstd = ops.instance_norm_forward(xc, weight, bias, eps)
        ctx.save_for_backward(xc, mean, rstd, weight)
        ctx.affine = (weight is not None and weight.requires_grad, bias is not None and bias.requires_grad)
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import ops

        x, mean, rstd, weight = ctx.saved_tensors
        dx, dg, db = ops.instance_norm_backward(x, dy.contiguous(), mean, rstd, weight, need_affine_grads=any(ctx.affine))
        return dx, (dg if ctx.affine[0] else None), (db if ctx.affine[1] else None), None


class _BatchNormTrainFn(torch.autograd.Function):
    """BatchNorm1d with BATCH statistics on [rows, E] (policy.train(), nn/ops.py:45-47): forward eamrl_batchnorm_train -- the
    kernels, and therefore the bits, of the native rollout's encoder --, backward eamrl_batchnorm_backward.  The running
    statistics are not touched here (the rollout updated them once for this forward)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, running=None):
        from . import ops

        y = x.clone(memory_format=torch.contiguous_format)          # the kernel normalises in place; x is kept for the backward
        # running = (running_mean, running_var, momentum): this forward is the step's only encoder pass (MoE policies) and
        # updates the running statistics as the rollout's pass would have
        rm, rv, mom = running if running is not None else (None, None, 0.0)
        _, mean, var = ops.batchnorm_train_(y, weight.detach(), bias.detach(), rm, rv, mom, eps)
        ctx.save_for_backward(x.contiguous(), mean, var, weight)
        ctx.eps = eps
        ctx.affine = weight.requires_grad or bias.requires_grad
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import ops

        x, mean, var, weight = ctx.saved_tensors
        dx, dg, db = ops.batchnorm_backward(x, dy.contiguous(), mean, var, weight.detach(), ctx.eps, need_affine_grads=ctx.affine)
        return dx, dg, db, None, None


class _SmallLinearFn(torch.autograd.Function):
    """The init embeddings' Linear(2 .. 8 -> E) on [rows, K] node features: forward eamrl_linear's tiny-K kernel (the rollout's
    own init embedding), weight / bias gradient eamrl_small_linear_wgrad.  The features are inputs: no input gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        from . import ops

        xc = x.contiguous()
        ctx.save_for_backward(xc)
        ctx.has_bias = bias is not None
        return ops.linear(xc, weight.detach(), None if bias is None else bias.detach())

    @staticmethod
    def backward(ctx, dy):
        from . import ops

        (x,) = ctx.saved_tensors
        dW, db = ops.small_linear_wgrad(dy.contiguous(), x, need_bias=ctx.has_bias)
        return None, dW, db


def _small_linear(x, weight, bias):
    """F.linear for the init embeddings; native where the features need no gradient (they are the instance)."""
    if (x.is_cuda and x.dtype == torch.float32 and not x.requires_grad and weight.shape[1] <= 8 and weight.is_contiguous()
            and os.environ.get("EAMRL_TORCH_INIT_EMBED", "0") != "1"):
        return _SmallLinearFn.apply(x, weight, bias)
    return F.linear(x, weight, bias)


class _LinearFn(torch.autograd.Function):
    """torch.nn.Linear (+ ReLU) of the training graph on the package's own GEMMs: forward eamrl_linear (the rollout's kernel),
    input gradient eamrl_linear on the transposed weight, weight / bias gradient eamrl_linear_wgrad.  hipBLASLt runs these fp32 shapes
    (rows = B * N, 128 .. 512 columns) at 29-40 TFLOP/s; the fp32-MFMA kernels here at 70-95."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, residual):
        from . import ops

        xc = x if x.stride(-1) == 1 else x.contiguous()
        y = ops.linear(xc, weight, bias, relu=relu, residual=None if residual is None else residual.contiguous())
        ctx.save_for_backward(xc, weight, y if relu else None)
        ctx.relu, ctx.has_bias = relu, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import ops

        x, weight, y = ctx.saved_tensors
        g = dy.contiguous()
        if ctx.relu:
            g = torch.ops.aten.threshold_backward(g, y, 0.0)
        # dx = g W as eamrl_linear on the transposed copy of W (out x in floats, a 3 us copy): the [out][in]-weight variant of
        # the GEMM kernel runs these shapes 30 % faster than the right-multiplication one (eamrl_matmul_right)
        dx = ops.linear(g, weight.t().contiguous()) if ctx.needs_input_grad[0] else None
        dW = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dW, db = ops.linear_wgrad(g, x, need_bias=ctx.has_bias)
        return dx, dW, db, None, (dy if ctx.needs_input_grad[4] else None)


def _linear(x, weight, bias=None, relu=False, residual=None):
    """[residual +] F.linear (+ F.relu) -- on the native GEMMs where they apply (CUDA fp32, both dims multiples of 128)."""
    if (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and weight.is_contiguous()
            and weight.shape[0] % 128 == 0 and weight.shape[1] % 128 == 0 and os.environ.get("EAMRL_TORCH_LINEAR", "0") != "1"):
        return _LinearFn.apply(x, weight, bias, relu, residual)
    y = F.linear(x, weight, bias)
    y = F.relu(y) if relu else y
    return y if residual is None else residual + y


class _SelfAttentionFn(torch.autograd.Function):
    """The encoder's multi-head self-attention on the packed projection qkv [B, N, 3E] ("b s (three h d)", as Wqkv writes it):
    forward eamrl_mha_encoder (the rollout's kernel), backward eamrl_mha_encoder_backward, which recomputes the softmax from
    qkv -- nothing but qkv is kept.  torch's scaled_dot_product_attention needs [B, H, N, D] operands (permuted copies in and
    out) and its flash backward takes 0.7 ms per layer at 1024 x 100 nodes.  Graphs of up to 1024 nodes: k_mha_encoder_bwd
    (one workgroup per instance) to 112 nodes, k_mha_encoder_bwd_mfma (one per instance and head) above."""

    @staticmethod
    def forward(ctx, qkv, num_heads):
        from . import ops

        q = qkv.contiguous()
        ctx.save_for_backward(q)
        ctx.H = num_heads
        return ops.mha_encoder(q, num_heads)

    @staticmethod
    def backward(ctx, dout):
        from . import ops

        (q,) = ctx.saved_tensors
        return ops.mha_encoder_backward(q, dout.contiguous(), ctx.H), None


def _self_attention(qkv, B, N, E, H):
    """qkv [B, N, 3E] -> [B, N, E]"""
    from . import ops

    if (qkv.is_cuda and qkv.dtype == torch.float32 and os.environ.get("EAMRL_TORCH_ATTENTION", "0") != "1"
            and ops.mha_encoder_backward_supported(N, E, H)):
        return _SelfAttentionFn.apply(qkv, H)
    q = qkv.view(B, N, 3, H, E // H).permute(2, 0, 3, 1, 4)
    return F.scaled_dot_product_attention(q[0], q[1], q[2]).permute(0, 2, 1, 3).reshape(B, N, E)


def _normalize(norm: nn.Module, x: torch.Tensor, training: bool, update_running: bool = False) -> torch.Tensor:
    """update_running: a training-mode batch norm also updates its running statistics (the graph's forward is the step's only
    encoder pass: MoE policies)."""
    n = norm.normalizer
    if isinstance(n, nn.BatchNorm1d):
        # Batch statistics when training, as the reference (nn/ops.py:45-47) and as the native rollout that drew the
        # actions (ops.batchnorm_train_); the running statistics were updated by that rollout, not again here.
        x2 = x.reshape(-1, x.size(-1))
        if training and x2.is_cuda and x2.dtype == torch.float32 and n.weight is not None and n.bias is not None and x2.size(-1) % 4 == 0 \
                and os.environ.get("EAMRL_TORCH_BATCHNORM", "0") != "1":
            running = None
            if update_running and n.running_mean is not None:
                running = (n.running_mean, n.running_var, 0.1 if n.momentum is None else n.momentum)
                n.num_batches_tracked.add_(1)
            y = _BatchNormTrainFn.apply(x2, n.weight, n.bias, float(n.eps), running)
        elif training:
            upd = update_running and n.running_mean is not None
            if upd:
                n.num_batches_tracked.add_(1)
            y = F.batch_norm(x2, n.running_mean if upd else None, n.running_var if upd else None, n.weight, n.bias, True,
                             (0.1 if n.momentum is None else n.momentum) if upd else 0.0, n.eps)
        else:
            y = F.batch_norm(x2, n.running_mean, n.running_var, n.weight, n.bias, False, 0.0, n.eps)
        return y.view_as(x)
    if (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and n.weight is not None and n.bias is not None
            and os.environ.get("EAMRL_TORCH_INSTANCE_NORM", "0") != "1"):
        return _InstanceNormFn.apply(x, n.weight, n.bias, float(n.eps))
    return F.instance_norm(x.permute(0, 2, 1), weight=n.weight, bias=n.bias, eps=n.eps).permute(0, 2, 1)


def init_embedding_autograd(policy, td):
    """The init embedding of the training graph [B, M, E] (differentiable w.r.t. the init-embedding weights)."""
    enc = policy.encoder
    ie = enc.init_embedding
    locs = td["locs"]
    native_init = locs.is_cuda and os.environ.get("EAMRL_TORCH_INIT_EMBED", "0") != "1"
    if policy.env_name == "tsp":
        h = _small_linear(locs, ie.init_embed.weight, ie.init_embed.bias)
    elif policy.env_name == "pdp":      # depot | pickups with their deliveries' coordinates | deliveries (init.py:347-372)
        half = (locs.shape[1] - 1) // 2
        pick, deliv = locs[:, 1:half + 1], locs[:, half + 1:]
        h = torch.cat((_small_linear(locs[:, :1], ie.init_embed_depot.weight, ie.init_embed_depot.bias),
                       _small_linear(torch.cat((pick, deliv), -1), ie.init_embed_pick.weight, ie.init_embed_pick.bias),
                       _small_linear(deliv, ie.init_embed_delivery.weight, ie.init_embed_delivery.bias)), 1)
    else:
        depot = _small_linear(locs[:, :1], ie.init_embed_depot.weight, ie.init_embed_depot.bias)
        if policy.env_name == "pctsp":
            feat = torch.cat((locs[:, 1:], td["expected_prize"][..., None], td["penalty"][..., 1:, None]), -1)
        elif policy.env_name == "op":
            feat = torch.cat((locs[:, 1:], td["prize"][..., 1:, None]), -1)
        elif policy.env_name == "cvrptw":
            feat = torch.cat((locs[:, 1:], td["demand"][..., None], td["time_windows"][..., 1:, :].float(),
                              td["durations"][..., 1:, None]), -1)
        else:
            feat = torch.cat((locs[:, 1:], td["demand"][..., None]), -1)
        h = torch.cat((depot, _small_linear(feat, ie.init_embed.weight, ie.init_embed.bias)), 1)
    if locs.is_cuda and not native_init:
        # (cross-check path, EAMRL_TORCH_INIT_EMBED=1) the VALUE of the rollout's own init embedding (its kernels' rounding), the
        # gradient of torch's expression above: x + (y - y) is exactly x.  By default `_small_linear` already IS the rollout's
        # kernel, so -- the Linears / attention / norms below being the rollout's kernels too -- the embeddings of this graph equal
        # the native encoder's bit for bit (test_training_graph_encoder_equals_native_encoder) and one encoder pass can serve
        # rollout and gradient.
        with torch.no_grad():
            h_native = ie(td)
        h = h_native + (h - h.detach())
    return h


class _HeteroAttentionFn(torch.autograd.Function):
    """The HAM encoder's heterogeneous attention on the packed projection proj [B, M, 6E] (q | k | v | qpair | qsame | qother):
    forward eamrl_hetero_mha (the rollout's kernel), backward eamrl_hetero_mha_backward, which recomputes the softmax from proj
    -- nothing but proj is kept."""

    @staticmethod
    def forward(ctx, proj, num_heads):
        from . import ops

        p = proj.contiguous()
        ctx.save_for_backward(p)
        ctx.H = num_heads
        return ops.hetero_mha(p, num_heads)

    @staticmethod
    def backward(ctx, dout):
        from . import ops

        (p,) = ctx.saved_tensors
        return ops.hetero_mha_backward(p, dout.contiguous(), ctx.H), None


def hetero_attention_torch(proj, H):
    """The same as a torch expression (zoo/ham/attention.py:227-479 restated on the shared k and v): depot 0, pickups 1..P,
    deliveries P+1..2P; a non-depot row's general, pair, same-role and other-role scores under one softmax.  The cross-check of
    the kernels (EAMRL_TORCH_ATTENTION=1) and the path of graphs above the native backward's bound."""
    B, M, E6 = proj.shape
    E = E6 // 6
    D, P = E // H, (M - 1) // 2
    c = 1.0 / math.sqrt(D)
    q, k, v, qp, qs, qo = (proj[..., i * E:(i + 1) * E].reshape(B, M, H, D).permute(0, 2, 1, 3) for i in range(6))
    idx = torch.arange(M, device=proj.device)
    role = (idx > 0).long() + (idx > P).long()
    partner = torch.where(role == 1, idx + P, torch.where(role == 2, idx - P, idx))
    nd = role != 0
    ninf = torch.full((), float("-inf"), dtype=proj.dtype, device=proj.device)
    zero = torch.zeros((), dtype=proj.dtype, device=proj.device)
    kt = k.transpose(-1, -2)
    s_gen = c * (q @ kt)
    s_pair = torch.where(nd, c * (torch.where(nd[:, None], qp, zero) * k[:, :, partner]).sum(-1), ninf)
    s_x = torch.where(role[:, None] == role[None, :], c * (torch.where(nd[:, None], qs, zero) @ kt),
                      c * (torch.where(nd[:, None], qo, zero) @ kt))
    s_x = torch.where(nd[:, None] & nd[None, :], s_x, ninf)
    a = torch.softmax(torch.cat((s_gen, s_x, s_pair[..., None]), -1), -1)
    heads = (a[..., :M] + a[..., M:2 * M]) @ v + a[..., 2 * M:] * v[:, :, partner]
    return heads.permute(0, 2, 1, 3).reshape(B, M, E)


def _hetero_attention(proj, H):
    """proj [B, M, 6E] -> [B, M, E]"""
    from . import ops

    B, M, E6 = proj.shape
    if (proj.is_cuda and proj.dtype == torch.float32 and os.environ.get("EAMRL_TORCH_ATTENTION", "0") != "1"
            and ops.hetero_mha_backward_supported(M, E6 // 6, H)):
        return _HeteroAttentionFn.apply(proj, H)
    return hetero_attention_torch(proj, H)


def _encode_autograd_ham(policy, td):
    """The HAM encoder (policy.GraphHeterogeneousAttentionEncoder) of the training graph: the [H, E, D] weights are packed into
    Linear weights inside the graph (their gradients come back through the reshapes), the GEMMs, the attention and the norms
    run on this library's kernels where they apply."""
    enc = policy.encoder
    h = init_embedding_autograd(policy, td)
    training = policy.training
    for layer in enc.layers:
        mha, ffn = layer[0].module, layer[2].module
        B, M, E = h.shape
        assert M % 2 == 1, "Graph size should have odd number of nodes"
        P = (M - 1) // 2
        pack = lambda names: torch.cat([getattr(mha, n).permute(0, 2, 1).reshape(-1, E) for n in names], 0)
        qkv = _linear(h, pack(("W_query", "W_key", "W_val")))
        pick = _linear(h[:, 1:P + 1].contiguous(), pack(("W1_query", "W2_query", "W3_query")))
        deliv = _linear(h[:, P + 1:].contiguous(), pack(("W4_query", "W5_query", "W6_query")))
        proj = torch.cat((qkv, torch.cat((qkv.new_zeros(B, 1, 3 * E), pick, deliv), 1)), -1)
        att = _hetero_attention(proj, mha.num_heads)
        h = _normalize(layer[1], _linear(att, mha.W_out.reshape(-1, mha.embed_dim).t().contiguous(), residual=h), training)
        if isinstance(ffn, nn.Linear):
            x = _linear(h, ffn.weight, ffn.bias, residual=h)
        else:
            x = _linear(_linear(h, ffn[0].weight, ffn[0].bias, relu=True), ffn[2].weight, ffn[2].bias, residual=h)
        h = _normalize(layer[3], x, training)
    return h


def has_moe_encoder(policy) -> bool:
    """Whether an encoder layer's feed-forward sublayer is a mixture of experts (policy.MoE)."""
    from .policy import MoE

    layers = getattr(getattr(getattr(policy, "encoder", None), "net", None), "layers", None)
    return layers is not None and any(isinstance(getattr(layer[2], "module", None), MoE) for layer in layers
                                      if isinstance(layer, nn.Sequential) and len(layer) > 2)


def has_noisy_moe_encoder(policy) -> bool:
    """has_moe_encoder, and one of the MoE layers adds gating noise in training mode."""
    from .policy import MoE

    return has_moe_encoder(policy) and any(isinstance(layer[2].module, MoE) and layer[2].module.noisy_gating
                                           for layer in policy.encoder.net.layers)


def moe_autograd(moe, h, training: bool):
    """MoE(h) of an encoder layer as a torch expression on the module's parameters: the reference's function (nn/moe.py:208-277
    -- noisy top-k gating with its 1e-2 floor, gates normalised over the selected experts with + 1e-6, gate-weighted sum of the
    selected experts' outputs; the load-balancing loss is multiplied by loss_coef = 0 there and not formed here).  Every expert
    runs on all rows and unselected experts carry a zero gate, so nothing synchronises with the host; the selection breaks
    ties towards the lower expert index, as the kernels do (a stable sort).  h [..., E] -> [..., E]."""
    x = h.reshape(-1, h.shape[-1])
    logits = x @ moe.w_gate
    if moe.noisy_gating and training:
        std = F.softplus(x @ moe.w_noise) + 1e-2
        logits = logits + torch.randn_like(logits) * std
    p = torch.softmax(logits, -1)
    top_p, top_i = torch.sort(p, dim=-1, descending=True, stable=True)
    top_p, top_i = top_p[:, :moe.k], top_i[:, :moe.k]
    top_g = top_p / (top_p.sum(1, keepdim=True) + 1e-6)
    gates = torch.zeros_like(p).scatter(-1, top_i, top_g)
    y = None
    for e, ex in enumerate(moe.experts):
        o = _linear(_linear(x, ex.lins[0].weight, ex.lins[0].bias, relu=True), ex.lins[1].weight, ex.lins[1].bias)
        o = gates[:, e:e + 1] * o
        y = o if y is None else y + o
    return y.view_as(h)


class _MoEExpertsFn(torch.autograd.Function):
    """The selected experts of an MoE sublayer and their gate-weighted sum on a given routing: forward eamrl_moe_experts_forward
    (the rollout's expert and combine kernels on row lists in ascending row order), backward eamrl_moe_experts_backward.  Only
    the selected (row, expert) pairs are computed and only their outputs [rows, k, 128] are kept; the hidden activations are
    recomputed in the backward by the forward's own tile code.

    apply(x [rows, 128], gates [rows, k], sel [rows, k] (any integer dtype), packs, *params) -> y [rows, 128], with params = the
    n_exp lins.0.weight, then the n_exp lins.0.bias, lins.1.weight, lins.1.bias, and packs = the operand dict of
    MoE.packed_experts_backward() for those parameters (None: packed here).  Gradients: x, gates and every parameter; an expert
    that received no row gets zeros, not None."""

    @staticmethod
    def forward(ctx, x, gates, sel, packs, *params):
        from . import ops

        n = len(params) // 4
        if packs is None:
            W1, b1, W2, b2 = (list(p.detach() for p in params[i * n:(i + 1) * n]) for i in range(4))
            packs = dict(ops.pack_moe_experts(W1, b1, W2, b2), **ops.pack_moe_experts_backward(W1, W2))
        xc, gc = x.contiguous(), gates.contiguous()
        y, state = ops.moe_experts_forward(xc, sel.to(torch.int8).contiguous(), gc, packs)
        ctx.save_for_backward(xc, gc, state)
        ctx.packs, ctx.n = packs, n
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import ops

        x, g, state = ctx.saved_tensors
        need = ctx.needs_input_grad
        n = ctx.n
        dx, dg, dW1, db1, dW2, db2 = ops.moe_experts_backward(dy.contiguous(), x, g, ctx.packs, state, need_dx=need[0], need_dg=need[1],
                                                              need_weight_grads=any(need[4:]))
        grads = [None] * (4 * n)
        if dW1 is not None:
            for i, t in enumerate((dW1, db1, dW2, db2)):
                for e in range(n):
                    if need[4 + i * n + e]:
                        grads[i * n + e] = t[e]
        return (dx, dg, None, None, *grads)


def moe_native_backward(moe, h) -> bool:
    """Whether the MoE sublayer of the training graph runs on `_MoEExpertsFn`: CUDA float32 tensors, unless
    EAMRL_MOE_NATIVE_BACKWARD=0 asks for the torch expression `moe_autograd`."""
    return (h.is_cuda and h.dtype == torch.float32 and moe.w_gate.is_cuda and moe.w_gate.dtype == torch.float32
            and os.environ.get("EAMRL_MOE_NATIVE_BACKWARD", "1") != "0")


def moe_autograd_native(moe, h, training: bool):
    """`moe_autograd` with the experts on the native sparse path: the gate is the same torch expression (the same draw from the
    same generator state, the same stable sort, so the same routing), the selected experts, their weighted sum and all their
    gradients are `_MoEExpertsFn` -- k experts' arithmetic and saved activations per row instead of num_experts'."""
    x = h.reshape(-1, h.shape[-1])
    logits = x @ moe.w_gate
    if moe.noisy_gating and training:
        std = F.softplus(x @ moe.w_noise) + 1e-2
        logits = logits + torch.randn_like(logits) * std
    p = torch.softmax(logits, -1)
    top_p, top_i = torch.sort(p, dim=-1, descending=True, stable=True)
    top_p, top_i = top_p[:, :moe.k], top_i[:, :moe.k]
    top_g = top_p / (top_p.sum(1, keepdim=True) + 1e-6)
    params = [getattr(ex.lins[i], nm) for i, nm in ((0, "weight"), (0, "bias"), (1, "weight"), (1, "bias")) for ex in moe.experts]
    return _MoEExpertsFn.apply(x, top_g, top_i, moe.packed_experts_backward(), *params).view_as(h)


def encode_autograd(policy, td):
    enc = policy.encoder
    from .policy import GraphHeterogeneousAttentionEncoder, MoE

    if isinstance(enc, GraphHeterogeneousAttentionEncoder):
        return _encode_autograd_ham(policy, td)
    h = init_embedding_autograd(policy, td)
    training = policy.training
    # an MoE policy's step runs the encoder once, here (graph_encoder_equals_native): rollout and gradient must see the same
    # gating noise.  This pass then also keeps the batch norms' running statistics, which the rollout's pass keeps otherwise.
    single = has_moe_encoder(policy)
    for layer in enc.net.layers:
        mha, ffn = layer[0].module, layer[2].module
        B, N, E = h.shape
        H = mha.num_heads
        att = _self_attention(_linear(h, mha.Wqkv.weight, mha.Wqkv.bias), B, N, E, H)
        h = _normalize(layer[1], _linear(att, mha.out_proj.weight, mha.out_proj.bias, residual=h), training, single)
        if isinstance(ffn, MoE):
            moe_fn = moe_autograd_native if moe_native_backward(ffn, h) else moe_autograd
            h = _normalize(layer[3], h + moe_fn(ffn, h, training), training, single)
            continue
        x = h
        for lin in ffn.lins[:-1]:
            x = _linear(x, lin.weight, lin.bias, relu=True)
        h = _normalize(layer[3], _linear(x, ffn.lins[-1].weight, ffn.lins[-1].bias, residual=h), training)
    return h


# ------------------------------------------------------------------------------------------------------------
# per-step states from the action sequence
# ------------------------------------------------------------------------------------------------------------
def _tsp_states(actions, M, multistart):
    """-> first [R,T], cur [R,T], step0 [T] bool (placeholder context), mask [R,T,M] (True = feasible)."""
    R, T = actions.shape
    onehot = F.one_hot(actions, M).to(torch.int32)
    visited_before = torch.cumsum(onehot, 1) - onehot          # exclusive prefix
    cur = torch.cat((actions[:, :1], actions[:, :-1]), 1)       # a_{t-1}; column 0 unused at the placeholder step
    first = actions[:, :1].expand(R, T)
    return first, cur, visited_before == 0


def _cvrp_states(actions, demand_rows, vcap, M):
    """-> cur [R,T], remaining capacity [R,T] before each step, mask [R,T,M] (cvrp/env.py:68-100,132-144)."""
    R, T = actions.shape
    N = M - 1
    dev = actions.device
    visited = torch.zeros(R, M, dtype=torch.bool, device=dev)
    used = torch.zeros(R, dtype=torch.float32, device=dev)
    cur = torch.zeros(R, dtype=torch.int64, device=dev)
    lim = vcap + 1e-5
    curs, rems, masks = [], [], []
    ar = torch.arange(R, device=dev)
    for t in range(T):
        blocked = visited[:, 1:] | ((demand_rows + used[:, None]) > lim[:, None])
        depot_blocked = (cur == 0) & (~blocked).any(-1)
        masks.append(~torch.cat((depot_blocked[:, None], blocked), 1))
        curs.append(cur)
        rems.append(vcap - used)
        a = actions[:, t]
        d = demand_rows[ar, (a - 1).clamp(0, N - 1)]
        used = (used + d) * (a != 0).float()
        visited = visited.clone()
        visited[ar, a] = True
        cur = a
    return torch.stack(curs, 1), torch.stack(rems, 1), torch.stack(masks, 1)


def _pctsp_states(actions, prize_rows, prize_required):
    """-> cur [R,T], prize still to collect (clamped at 0) [R,T], mask [R,T,M] before each step
    (pctsp/env.py:64-97,156-163; context.py:194-208).  prize_rows [R, M] with a zero depot slot."""
    R, T = actions.shape
    M = prize_rows.shape[1]
    dev = actions.device
    visited = torch.zeros(R, M, dtype=torch.bool, device=dev)
    total = torch.zeros(R, dtype=torch.float32, device=dev)
    cur = torch.zeros(R, dtype=torch.int64, device=dev)
    curs, rems, masks = [], [], []
    ar = torch.arange(R, device=dev)
    for t in range(T):
        blocked = visited[:, 1:] | visited[:, :1]
        depot_blocked = (total < 1.0) & (~visited[:, 1:]).any(-1)
        masks.append(~torch.cat((depot_blocked[:, None], blocked), 1))
        curs.append(cur)
        rems.append((prize_required - total).clamp(min=0))
        a = actions[:, t]
        total = total + prize_rows[ar, a]
        visited = visited.clone()
        visited[ar, a] = True
        cur = a
    return torch.stack(curs, 1), torch.stack(rems, 1), torch.stack(masks, 1)


def _pdp_states(actions, available, to_deliver, mask0):
    """-> cur [R,T], mask [R,T,M] before each step (pdp/env.py:66-106), replayed from the rows' reset state: available and
    to_deliver [R,M] bool, mask0 the reset mask (with force_start_at_depot it is not their AND).  The partner index keeps the
    reference's modulo: (a + N/2) % (N + 1)."""
    R, T = actions.shape
    M = available.shape[1]
    dev = actions.device
    cur = torch.zeros(R, dtype=torch.int64, device=dev)
    ar = torch.arange(R, device=dev)
    curs, masks = [], []
    mask = mask0
    for t in range(T):
        masks.append(mask)
        curs.append(cur)
        a = actions[:, t]
        available, to_deliver = available.clone(), to_deliver.clone()
        available[ar, a] = False
        to_deliver[ar, (a + (M - 1) // 2) % M] = True
        mask = available & to_deliver
        cur = a
    return torch.stack(curs, 1), torch.stack(masks, 1)


def _cvrptw_states(actions, demand_rows, vcap, locs_rows, tw_rows, dur_rows):
    """-> cur [R,T], free capacity [R,T], clock [R,T], mask [R,T,M] before each step (cvrptw/env.py:103-138).
    tw_rows [R,M,2] and dur_rows [R,M] as float32."""
    R, T = actions.shape
    M = locs_rows.shape[1]
    N = M - 1
    dev = actions.device
    visited = torch.zeros(R, M, dtype=torch.bool, device=dev)
    used = torch.zeros(R, dtype=torch.float32, device=dev)
    now = torch.zeros(R, dtype=torch.float32, device=dev)
    cur = torch.zeros(R, dtype=torch.int64, device=dev)
    lim = vcap + 1e-5
    curs, rems, nows, masks = [], [], [], []
    ar = torch.arange(R, device=dev)
    for t in range(T):
        blocked = visited[:, 1:] | ((demand_rows + used[:, None]) > lim[:, None])
        depot_blocked = (cur == 0) & (~blocked).any(-1)
        dist = (locs_rows[ar, cur][:, None, :] - locs_rows).norm(p=2, dim=-1)
        in_time = now[:, None] + dist <= tw_rows[..., 1]
        masks.append(~torch.cat((depot_blocked[:, None], blocked), 1) & in_time)
        curs.append(cur)
        rems.append(vcap - used)
        nows.append(now)
        a = actions[:, t]
        now = (a != 0).float() * (torch.maximum(now + dist[ar, a], tw_rows[ar, a, 0]) + dur_rows[ar, a])
        used = (used + demand_rows[ar, (a - 1).clamp(0, N - 1)]) * (a != 0).float()
        visited = visited.clone()
        visited[ar, a] = True
        cur = a
    return torch.stack(curs, 1), torch.stack(rems, 1), torch.stack(nows, 1), torch.stack(masks, 1)


def _op_states(actions, locs_rows, maxlen_rows):
    """-> cur [R,T], length still allowed to the depot's limit [R,T], mask [R,T,M] before each step
    (op/env.py:69-102,149-165; context.py:211-223).  locs_rows [R,M,2], maxlen_rows [R,M]."""
    R, T = actions.shape
    M = locs_rows.shape[1]
    dev = actions.device
    visited = torch.zeros(R, M, dtype=torch.bool, device=dev)
    length = torch.zeros(R, dtype=torch.float32, device=dev)
    cur = torch.zeros(R, dtype=torch.int64, device=dev)
    curs, rems, masks = [], [], []
    ar = torch.arange(R, device=dev)
    for t in range(T):
        here = locs_rows[ar, cur]
        exceeds = length[:, None] + (locs_rows - here[:, None, :]).norm(p=2, dim=-1) > maxlen_rows
        m = ~(visited | visited[:, :1] | exceeds)
        m[:, 0] = True
        masks.append(m)
        curs.append(cur)
        rems.append(maxlen_rows[:, 0] - length)
        a = actions[:, t]
        length = length + (locs_rows[ar, a] - here).norm(p=2, dim=-1)
        visited = visited.clone()
        visited[ar, a] = True
        cur = a
    return torch.stack(curs, 1), torch.stack(rems, 1), torch.stack(masks, 1)


def _sdvrp_states(actions, demand_rows, vcap, M):
    """-> cur [R,T], free capacity [R,T], mask [R,T,M] and remaining demand [R,T,M] before each step
    (sdvrp/env.py:58-92,137-146)."""
    R, T = actions.shape
    dev = actions.device
    rem = torch.cat((torch.zeros(R, 1, dtype=torch.float32, device=dev), demand_rows), 1)
    used = torch.zeros(R, dtype=torch.float32, device=dev)
    cur = torch.zeros(R, dtype=torch.int64, device=dev)
    curs, frees, masks, rems = [], [], [], []
    ar = torch.arange(R, device=dev)
    for t in range(T):
        blocked = (rem[:, 1:] == 0) | (used >= vcap)[:, None]
        depot_blocked = (cur == 0) & (~blocked).any(-1)
        masks.append(~torch.cat((depot_blocked[:, None], blocked), 1))
        curs.append(cur)
        frees.append(vcap - used)
        rems.append(rem)
        a = actions[:, t]
        delivered = torch.minimum(rem[ar, a], vcap - used)
        used = (used + delivered) * (a != 0).float()
        rem = rem.clone()
        rem[ar, a] = rem[ar, a] - delivered
        cur = a
    return torch.stack(curs, 1), torch.stack(frees, 1), torch.stack(masks, 1), torch.stack(rems, 1)


# ------------------------------------------------------------------------------------------------------------
# differentiable decoder inputs and the per-chunk log-probabilities
# ------------------------------------------------------------------------------------------------------------
_STATE_KEYS = {name: spec.reeval_static for name, spec in ENV_SPECS.items()}


class shared_decoder_tensors:
    """Within this context, policy calls on the SAME instances under the SAME parameters share one differentiable
    encoder pass (`decoder_tensors`) and one native encoder + cache launch (`AttentionModelPolicy._enqueue`): the EAM
    step evaluates the sampled and the improved tours of a batch one after the other (zoo/earl/model.py:179-195 runs the
    whole policy, encoder included, twice), and both losses are summed before the one backward -- so one encoder graph
    serves both, with identical gradients up to summation order.  Opt-in, because a graph that has already been
    backpropagated through cannot serve a second backward."""

    def __init__(self, policy):
        self.policy = policy

    def __enter__(self):
        self.policy._shared_dt = {}
        return self

    def __exit__(self, *exc):
        self.policy._shared_dt = None
        return False


def _graph_key(policy, td):
    """Identity of (instances, parameters, mode): storage address, in-place version and shape of every input tensor, the sums
    of the same over the parameters (an optimizer step or load_state_dict changes them) and, in eval mode, the buffers (the
    running statistics of batch norm are read only then; in train mode every native rollout updates them in place)."""
    ins = tuple((k, v.data_ptr(), v._version, tuple(v.shape)) for k, v in sorted(td.items(), key=lambda kv: kv[0])
                if torch.is_tensor(v))
    # (walking the module tree costs 0.3 ms per call and a step asks several times: the lists of Parameter / buffer objects
    # are kept -- .to(), load_state_dict and optimizer steps keep the objects; the key is only ever compared within one step)
    lists = policy.__dict__.get("_key_tensors")
    if lists is None:
        lists = (list(policy.parameters()), list(policy.buffers()))
        policy.__dict__["_key_tensors"] = lists
    ver = ptr = 0
    for p_ in lists[0] + ([] if policy.training else lists[1]):
        ver += p_._version
        ptr += p_.data_ptr()
    return ins, ver, ptr, policy.training, torch.is_grad_enabled()


def graph_encoder_equals_native(policy, td) -> bool:
    """True where `encode_autograd` reproduces the native encoder's embeddings bit for bit AND may stand in for it: instance-norm
    layers (their training forward kernel sums in the rollout's order), every Linear, the self-attention and the norms on this
    library's kernels (none of the EAMRL_TORCH_* switches), fp32 on the GPU.  Batch-norm policies keep two passes: their graph
    runs on the same kernels since round 3 (`_BatchNormTrainFn`), but the rollout's pass is the one that updates the running
    statistics.  Graphs of up to 1024 nodes, where the self-attention's backward is native (the native re-evaluation's limit
    too); above that the graph's attention is torch's.
    MoE policies (`has_moe_encoder`) are the exception: the answer is True on fp32 GPU tensors whatever the norm and whatever the
    EAMRL_TORCH_* / EAMRL_SEPARATE_ENCODER_PASSES switches say.  Their graph does NOT reproduce the native bits (the MoE
    sublayer is a torch expression there); it stands in for the native encoder because rollout and gradient must see one draw
    of the gating noise."""
    from . import ops

    locs = td["locs"]
    if has_moe_encoder(policy):
        # MoE policies: the graph's embeddings are not the native encoder's bits (its MoE sublayer is a torch expression), but
        # they MUST stand in for them -- with noisy gating a second pass would draw other noise and route rows differently, so
        # the rollout's log-likelihood and its gradient would belong to different networks.  Any norm, any switch.
        return bool(locs.is_cuda and locs.dtype == torch.float32)
    if any(os.environ.get(k, "0") == "1" for k in ("EAMRL_TORCH_LINEAR", "EAMRL_TORCH_ATTENTION", "EAMRL_TORCH_INSTANCE_NORM",
                                                  "EAMRL_SEPARATE_ENCODER_PASSES")):
        return False
    enc = getattr(policy, "encoder", None)
    layers = getattr(getattr(enc, "net", None), "layers", None)
    if layers is None or not locs.is_cuda or locs.dtype != torch.float32:
        return False
    for layer in layers:
        mha, ffn = layer[0].module, layer[2].module
        E = mha.Wqkv.weight.shape[1]
        if E != 128 or mha.num_heads != 8 or len(ffn.lins) != 2 or ffn.lins[0].weight.shape[0] % 128 \
                or not ops.mha_encoder_backward_supported(locs.shape[1], E, mha.num_heads):
            return False
        for norm in (layer[1], layer[3]):
            n = norm.normalizer
            if not isinstance(n, nn.InstanceNorm1d) or n.weight is None or n.bias is None:
                return False
    return True


def decoder_tensors(policy, td):
    """The differentiable tensors the decode steps read: node embeddings, glimpse key / value, logit key, graph
    context (encoder + `_precompute_cache` with autograd) and the decoder's own parameters.  -> dict name -> tensor."""
    shared = getattr(policy, "_shared_dt", None)
    key = None
    if shared is not None:
        key = _graph_key(policy, td)
        ent = shared.get("graph")
        if ent is not None and ent[0] == key:
            return ent[1]
    dec = policy.decoder
    emb = encode_autograd(policy, td)
    K, V, L = _linear(emb, dec.project_node_embeddings.weight).chunk(3, dim=-1)
    t = {"emb": emb, "K": K, "V": V, "L": L, "Wctx": dec.context_embedding.project_context.weight,
         "Wout": dec.pointer.project_out.weight}
    if dec.use_graph_context:
        t["gctx"] = F.linear(emb.mean(1), dec.project_fixed_context.weight)
    if policy.env_name == "tsp":
        t["placeholder"] = dec.context_embedding.W_placeholder
    if policy.env_name == "sdvrp":
        t["dyn"] = dec.dynamic_embedding.projection.weight
    if getattr(dec, "is_polynet", False):      # PolyNetAttention's layers (nn/attention.py:516-517) and its strategy table
        ptr = dec.pointer
        t.update(polyW1=ptr.poly_layer_1.weight, polyb1=ptr.poly_layer_1.bias, polyW2=ptr.poly_layer_2.weight,
                 polyb2=ptr.poly_layer_2.bias, polyZ=ptr.binary_vectors)
    if shared is not None:
        shared["graph"] = (key, t)
    return t


def _filter_logits_(logits, act, top_k: int, top_p: float):
    """process_logits' top-k / top-p filtering (utils/decoding.py:111-137,170-176) as a fixed, non-differentiated choice of the
    entries that stay: top-k keeps an entry iff fewer than k are strictly larger, top-p sorts ascending and drops the entries
    whose cumulative probability stays <= 1 - top_p.  The chosen action always stays (it did in the rollout;
    a last-bit difference between torch's sums and the rollout kernel's at the threshold must not turn its log-prob into -inf)."""
    with torch.no_grad():
        drop = torch.zeros_like(logits, dtype=torch.bool)
        if top_k > 0:
            k = min(int(top_k), logits.shape[-1])
            kth = torch.topk(logits, k, dim=-1).values[..., -1:]
            drop |= logits < kth
        if 0.0 < top_p < 1.0:
            x = logits.masked_fill(drop, float("-inf"))
            srt, idx = torch.sort(x, dim=-1, descending=False, stable=True)
            cum = torch.softmax(srt, dim=-1).cumsum(-1)
            thr = torch.tensor(1.0 - float(top_p), dtype=torch.float32).item()     # float32(1 - top_p): the double rounded once
            drop |= torch.zeros_like(drop).scatter_(-1, idx, cum <= thr)
        drop.scatter_(-1, act[..., None], False)
    return logits.masked_fill(drop, float("-inf"))


def _logp_rows(env_name, t, static, act, nrep, multistart, H, temperature, clip, top_k=0, top_p=0.0, s_first=0,
               return_entropy=False):
    """Per-step log-probabilities [Rc, T] of the rows `act` (nrep whole start groups of the B instances, (s b) order).
    `t`: decoder_tensors; `static`: the instance tensors the masks are rebuilt from.  s_first: index of the rows' first start
    group in the whole rollout (PolyNet: the strategy of a row is its start index modulo k).
    return_entropy: -> (logp, entropy [Rc, T]), the entropy of every step's distribution from the same log-softmax
    (calculate_entropy, rl4co/utils/ops.py:108-116, before its sum over the steps; 0 for the multistart column)."""
    emb, K, V, L = t["emb"], t["K"], t["V"], t["L"]
    B, M, E = emb.shape
    D = E // H
    rep = lambda x: x.repeat(nrep, *([1] * (x.dim() - 1)))   # (s b) order: instance index = row % B
    embr, Kr, Vr, Lr = rep(emb), rep(K), rep(V), rep(L)
    Rc, T = act.shape
    ar = torch.arange(Rc, device=act.device)[:, None]
    dem_t = None
    with torch.no_grad():
        if env_name == "tsp":
            first, cur, mask = _tsp_states(act, M, multistart)
            rem = now = None
        elif env_name == "pdp":
            cur, mask = _pdp_states(act, rep(static["available"]), rep(static["to_deliver"]), rep(static["action_mask"]))
            rem = now = None
        elif env_name == "cvrptw":
            cur, rem, now, mask = _cvrptw_states(act, rep(static["demand"]), rep(static["vehicle_capacity"].reshape(-1)),
                                                 rep(static["locs"]), rep(static["time_windows"].float()),
                                                 rep(static["durations"].float()))
        elif env_name == "op":
            cur, rem, mask = _op_states(act, rep(static["locs"]), rep(static["max_length"]))
        elif env_name == "pctsp":
            cur, rem, mask = _pctsp_states(act, rep(static["real_prize"]), rep(static["prize_required"].reshape(-1)))
        elif env_name == "cvrp":
            cur, rem, mask = _cvrp_states(act, rep(static["demand"]), rep(static["vehicle_capacity"].reshape(-1)), M)
        else:
            cur, rem, mask, dem_t = _sdvrp_states(act, rep(static["demand"]), rep(static["vehicle_capacity"].reshape(-1)), M)
    if env_name == "tsp":
        ctx_in = torch.cat((embr[ar, first], embr[ar, cur]), -1)                       # [Rc, T, 2E]
        if not multistart:   # step 0 uses the learned placeholder (context.py:118-131)
            ctx_in = torch.cat((t["placeholder"].expand(Rc, 1, 2 * E), ctx_in[:, 1:]), 1)
    elif env_name == "pdp":
        ctx_in = embr[ar, cur]                                                           # [Rc, T, E]  (context.py:242-253)
    elif env_name == "cvrptw":
        ctx_in = torch.cat((embr[ar, cur], rem[..., None], now[..., None]), -1)          # [Rc, T, E+2]
    else:
        ctx_in = torch.cat((embr[ar, cur], rem[..., None]), -1)                          # [Rc, T, E+1]
    q = F.linear(ctx_in, t["Wctx"])
    if "gctx" in t:
        q = q + rep(t["gctx"])[:, None, :]
    qh = q.view(Rc, T, H, D).permute(0, 2, 1, 3)
    kh = Kr.view(Rc, M, H, D).permute(0, 2, 1, 3)
    vh = Vr.view(Rc, M, H, D).permute(0, 2, 1, 3)
    if env_name == "sdvrp":
        # dynamic embedding (dynamic.py:59-78): K/V/L rows + remaining demand * projection columns.  The update is
        # rank one, so it enters as a score bias and two outer products instead of [Rc, T, M, E] tensors
        wk, wv, wl = t["dyn"].view(3, E)
        qw = (qh * wk.view(1, H, 1, D)).sum(-1)                                              # [Rc, H, T]
        bias = (dem_t[:, None] * qw[..., None]) / math.sqrt(D)                               # [Rc, H, T, M]
        bias = bias.masked_fill(~mask[:, None], float("-inf"))
        att = torch.softmax(torch.matmul(qh, kh.transpose(-1, -2)) / math.sqrt(D) + bias, dim=-1)
        heads = torch.matmul(att, vh) + (att * dem_t[:, None]).sum(-1, keepdim=True) * wv.view(1, H, 1, D)
    else:
        heads = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask[:, None])     # [Rc, H, T, D]
    hcat = heads.permute(0, 2, 1, 3).reshape(Rc, T, E)
    if "eas_layer" in t:    # EAS-Lay (zoo/eas/decoder.py:12-32): a callable on the concatenated heads [Rc, T, E], before project_out
        hcat = t["eas_layer"](hcat)
    glimpse = F.linear(hcat, t["Wout"])
    if "polyW1" in t:       # PolyNetAttention.forward (nn/attention.py:534-545): row r = s * B + b uses strategy (s_first + s) % k
        Z = t["polyZ"]
        z = Z[(s_first + torch.arange(Rc, device=act.device) // B) % Z.shape[0]]
        hid = F.relu(F.linear(torch.cat((glimpse, z[:, None, :].expand(Rc, T, z.shape[-1])), -1), t["polyW1"], t["polyb1"]))
        glimpse = glimpse + F.linear(hid, t["polyW2"], t["polyb2"])
    logits = torch.bmm(glimpse, Lr.transpose(1, 2))
    if env_name == "sdvrp":
        logits = logits + dem_t * (glimpse @ wl)[..., None]
    logits = logits / math.sqrt(E)
    if clip > 0:
        logits = torch.tanh(logits) * clip
    logits = logits.masked_fill(~mask, float("-inf")) / temperature
    if top_k > 0 or 0.0 < top_p < 1.0:
        logits = _filter_logits_(logits, act, top_k, top_p)
    lsm = F.log_softmax(logits, dim=-1)
    logp = lsm.gather(-1, act[..., None]).squeeze(-1)
    if multistart:   # the start node is not a decision (decoding.py:318-324)
        logp = torch.cat((torch.zeros_like(logp[:, :1]), logp[:, 1:]), 1)
        # steps t >= 1 were evaluated with the state after the start action: column t uses prefix a_{<t} as built
    if return_entropy:      # infeasible nodes: log p = -inf, p = 0 -> their term is 0 (nan_to_num in the reference), no 0 * inf
        lp = lsm.masked_fill(~mask, 0.0)
        ent = -(lp.exp().masked_fill(~mask, 0.0) * lp).sum(-1)
        if multistart:
            ent = torch.cat((torch.zeros_like(ent[:, :1]), ent[:, 1:]), 1)
        return logp, ent
    return logp


class _ChunkedReeval(torch.autograd.Function):
    """logp = cat_c fn(c, *tensors) with activation memory bounded to one chunk: the forward keeps no graph, the
    backward recomputes each chunk with autograd and accumulates the gradients of `tensors`."""

    @staticmethod
    def forward(ctx, fn, n_chunks, *tensors):
        with torch.no_grad():
            outs = [fn(c, *tensors) for c in range(n_chunks)]
        ctx.fn, ctx.n_chunks = fn, n_chunks
        ctx.save_for_backward(*tensors)
        return torch.cat(outs, 0)

    @staticmethod
    def backward(ctx, g):
        leaves = [x.detach().requires_grad_(need) for x, need in zip(ctx.saved_tensors, ctx.needs_input_grad[2:])]
        need = [x for x in leaves if x.requires_grad]
        acc = [None] * len(need)
        off = 0
        for c in range(ctx.n_chunks):
            with torch.enable_grad():
                out = ctx.fn(c, *leaves)
            gs = torch.autograd.grad(out, need, g[off:off + out.shape[0]], allow_unused=True)
            off += out.shape[0]
            for i, gi in enumerate(gs):
                if gi is not None:
                    acc[i] = gi if acc[i] is None else acc[i].add_(gi)
        it = iter(acc)
        return (None, None) + tuple(next(it) if x.requires_grad else None for x in leaves)


# ------------------------------------------------------------------------------------------------------------
# native (HIP) re-evaluation: forward and backward of all decode steps on fp32 MFMA (csrc/reeval.hip)
# ------------------------------------------------------------------------------------------------------------
_NATIVE_ENVS = ("tsp", "cvrp", "pctsp", "op", "cvrptw", "sdvrp")      # PDP: the PyTorch re-evaluation path (`_pdp_states`)


def native_reeval_supported(policy, M: int) -> bool:
    import os

    from . import ops

    dec = policy.decoder
    if getattr(dec, "is_polynet", False):       # the re-evaluation kernels have no PolyNet layers: the PyTorch expression
        return False
    return (os.environ.get("EAMRL_NATIVE_REEVAL", "1") != "0" and policy.env_name in _NATIVE_ENVS
            and ops.reeval_supported(M, dec.embed_dim, dec.num_heads))


@torch.no_grad()
def replay_states(policy, td, actions, S: int, multistart: bool):
    """What the env state is before every decode step of the given action rows, in the form the re-evaluation kernels
    read it: mask bits [R, T, 4], the node(s) whose folded context rows enter the query (idxA / idxB [R, T], -1 = none) and
    the state scalars sc [NC, R, T] multiplying the state columns of project_context.  TSP is closed-form in the
    actions; the other envs replay their transition kernels step by step (eamrl_*_step_mask + eamrl_pack_mask_bits).
    -> dict(maskbits, idxA, idxB, sc, tstart, placeholder)"""
    from . import ops
    from .policy import _env_step_, state_from_td

    env_name = policy.env_name
    R, T = actions.shape
    dev = actions.device
    actions = actions.contiguous()
    if env_name == "tsp":
        M = td["locs"].shape[1]
        bits = ops.tsp_mask_bits(actions, M) if M <= ops.KEY_CHUNK else ops.tsp_mask_bits_chunked(actions, M)
        a32 = actions.to(torch.int32)
        prev = torch.cat((torch.full((R, 1), -1, dtype=torch.int32, device=dev), a32[:, :-1]), 1)       # a_{t-1}
        first = a32[:, :1].expand(R, T).contiguous()
        sc, placeholder = None, False
        if not multistart:       # step 0: the learned placeholder replaces both gathered rows (context.py:118-131)
            first = first.clone()
            first[:, 0] = -1
            sc = torch.zeros(1, R, T, dtype=torch.float32, device=dev)
            sc[0, :, 0] = 1.0
            placeholder = True
        return dict(maskbits=bits, idxA=first, idxB=prev.contiguous(), sc=sc, tstart=1 if multistart else 0,
                    placeholder=placeholder)
    B = td["action_mask"].shape[0]
    if env_name == "sdvrp":     # + the remaining demands of every step (the dynamic embedding's input)
        st = state_from_td(env_name, td, S, copy=False)
        bits, idxA, sc, rem = ops.replay_states_sdvrp(st, actions)
        return dict(maskbits=bits, idxA=idxA, idxB=None, sc=sc, tstart=1 if multistart else 0, placeholder=False, rem=rem)
    big = td["action_mask"].shape[-1] > ops.KEY_CHUNK            # key-chunked kernels: their mask layout (either way)
    if os.environ.get("EAMRL_REPLAY_LOOP", "0") != "1":         # one launch: the env's transitions replayed inside a kernel
        st = state_from_td(env_name, td, S, copy=False)         # read-only
        bits, idxA, sc = ops.replay_states(st, actions, B)
        return dict(maskbits=bits, idxA=idxA, idxB=None, sc=sc, tstart=1 if multistart else 0, placeholder=False)
    st = state_from_td(env_name, td, S)                         # (the step-by-step form, kept as the cross-check)
    NC = ENV_SPECS[env_name].n_state_cols
    bits = torch.empty((R, T, -(-st.M // ops.KEY_CHUNK), 4) if big else (R, T, 4), dtype=torch.int32, device=dev)
    idxA = torch.empty(R, T, dtype=torch.int32, device=dev)
    sc = torch.empty(NC, R, T, dtype=torch.float32, device=dev)
    for t in range(T):
        (ops.pack_mask_bits_chunked_ if big else ops.pack_mask_bits_)(st.mask, bits, t)
        idxA[:, t] = st.cur
        if env_name == "pctsp":          # prize still to collect, clamped at 0 (context.py:194-208)
            sc[0, :, t] = (st.vcap - st.used).clamp_(min=0)
        else:                            # free capacity (cvrp, cvrptw) / length still allowed (op: vcap = max_length[:, 0])
            sc[0, :, t] = st.vcap - st.used
        if env_name == "cvrptw":
            sc[1, :, t] = st.time
        _env_step_(st, actions[:, t].contiguous())
    return dict(maskbits=bits, idxA=idxA, idxB=None, sc=sc, tstart=1 if multistart else 0, placeholder=False)


class _NativeReeval(torch.autograd.Function):
    """logp [R, T] = eamrl_reeval_forward(K, V, Lp, Pa, Pb, gctx, cvec | replayed states); backward = eamrl_reeval_backward.
    meta["want_entropy"]: -> (logp [R, T], entropy [R, T]), and both upstream gradients go into ONE backward call
    (eamrl_reeval.glogp / .gent)."""

    @staticmethod
    def forward(ctx, K, V, Lp, Pa, Pb, gctx, cvec, meta, dyn=None):
        from . import ops

        want_entropy = bool(meta.get("want_entropy"))
        parts = [K, V, Lp, Pa] + ([Pb] if Pb is not None else [])
        buf = torch.cat([x.detach() for x in parts], -1).contiguous()
        plan = ops.ReevalPlan(buf, Pb is not None, None if gctx is None else gctx.detach().contiguous(),
                              None if cvec is None else cvec.detach().contiguous(), meta["idxA"], meta["idxB"], meta["sc"],
                              meta["maskbits"], meta["actions"], meta["S"], meta["tstart"], meta["clip"], meta["temp"],
                              rollout_logp=meta.get("rollout_logp"), rollout_heads=meta.get("rollout_heads"),
                              rem=meta.get("rem"), dyn=None if dyn is None else dyn.detach().contiguous(),
                              want_entropy=want_entropy)
        ctx.plan = plan
        ctx.has = (Pb is not None, gctx is not None, cvec is not None, dyn is not None)
        logp = plan.forward()
        if want_entropy:
            ctx.set_materialize_grads(False)        # an unused output hands None to the backward, not a tensor of zeros
            return logp, plan.entropy.view_as(plan.entropy)
        return logp

    @staticmethod
    def backward(ctx, g, gent=None):
        plan = ctx.plan
        if g is None:
            g = torch.zeros(plan.R, plan.T, dtype=torch.float32, device=plan.buf.device)
        dbuf, dg, dc = plan.backward(g, gent)
        plan.heads = None           # 5 .. 10 GB at the POMO sizes: not kept for as long as the graph object lives
        E = plan.E
        sl = [dbuf[..., i * E:(i + 1) * E] for i in range(5 if ctx.has[0] else 4)]
        return (sl[0], sl[1], sl[2], sl[3], sl[4] if ctx.has[0] else None, dg if ctx.has[1] else None,
                dc if ctx.has[2] else None, None, plan.ddyn if ctx.has[3] else None)


def _evaluate_native(policy, t, td, actions, S, multistart, temperature, clip, rollout_logp=None, rollout_heads=None,
                     return_entropy=False):
    """Differentiable log-probs [R, T]: the weight folds (Lp = L Wout, Pa / Pb = emb x halves of project_context, state
    columns) as small autograd GEMMs on the decoder tensors `t`, everything per (row, step) in the HIP kernels.
    return_entropy: -> (logp, entropy [R, T]), both with a graph (single-chunk graphs: the backward kernel's limit)."""
    E = t["emb"].shape[-1]
    Wctx = t["Wctx"]
    Lp = _linear(t["L"], t["Wout"].t().contiguous())
    Pa = _linear(t["emb"], Wctx[:, :E].contiguous())
    Pb = _linear(t["emb"], Wctx[:, E:2 * E].contiguous()) if policy.env_name == "tsp" else None
    meta = replay_states(policy, td, actions, S, multistart)
    if policy.env_name == "tsp":
        cvec = F.linear(t["placeholder"][None], Wctx) if meta["placeholder"] else None            # [1, E]
    else:
        cvec = Wctx[:, E:].t()                                                                      # [NC, E] state columns
    meta.update(actions=actions.contiguous(), S=S, clip=float(clip), temp=float(temperature), want_entropy=bool(return_entropy))
    if return_entropy:          # the forward kernel always runs: the backward reads its lse and entropy
        rollout_logp = None
    if rollout_logp is not None:
        meta["rollout_logp"] = rollout_logp.detach().to(torch.float32).contiguous()
        if rollout_heads is not None:           # the rollout kernel's glimpse outputs of these very steps: not recomputed
            meta["rollout_heads"] = rollout_heads.detach()
    dyn = None
    if policy.env_name == "sdvrp":      # wk | wv | lw: the logit-key column folded through project_out like Lp (dynamic.py:59-78)
        wk, wv, wl = t["dyn"].view(3, E)
        dyn = torch.stack((wk, wv, wl @ t["Wout"]))
    return _NativeReeval.apply(t["K"], t["V"], Lp, Pa, Pb, t.get("gctx"), cvec, meta, dyn)


def evaluate_log_likelihood(policy, td, env, actions, num_starts: int = 0, temperature=None, tanh_clipping=None,
                            chunk_rows: int = 4096, multistart=None, checkpoint=None, native=None, rollout_logp=None,
                            rollout_heads=None, top_k: int = 0, top_p: float = 0.0, return_entropy: bool = False):
    """Differentiable per-step log-probabilities of `actions` [R, T] (R = B or S*B rows in (s b) order).  native
    (default: where supported -- TSP / CVRP / PCTSP / OP / CVRPTW, graphs up to 112 nodes): forward and backward of the
    decode steps run in the HIP re-evaluation kernels; otherwise (and as the cross-check) PyTorch autograd ops.  multistart
    (default: num_starts > 1): the first column is the start node and gets log-prob 0; False with num_starts > 1 is
    the multi-sample layout (every column a decision).  checkpoint (default: by size): keep no activations in the
    forward and recompute chunk by chunk in the backward.  rollout_logp [R, T] (native path only): the per-step log-probs
    the rollout kernel produced for exactly these actions with this policy -- the HIP forward pass is then skipped (the
    returned values are these; the backward recovers each step's normaliser from them).  top_k / top_p: the rollout filtered
    its logits (process_logits, decoding.py:170-176): the same entries are dropped here, as a fixed mask, before the
    log-softmax (PyTorch path).  Returns logp [R, T]; with return_entropy=True (logp, entropy [R, T]) -- each step's
    calculate_entropy term (rl4co/utils/ops.py:108-116, before the sum over the steps), with a graph like logp: from the HIP
    kernels where they serve the shape (up to 112 nodes: the entropy gradient is not built for key chunks), from the PyTorch
    path's log-softmax otherwise.  Not under top_k / top_p (NotImplementedError)."""
    if return_entropy and (top_k > 0 or 0.0 < top_p < 1.0):
        raise NotImplementedError("evaluate_log_likelihood: a differentiable entropy under top_k / top_p is not built "
                                  "(the entropy of a filtered distribution stays the rollout's step loop)")
    temperature = policy.temperature if temperature is None else temperature
    clip = policy.tanh_clipping if tanh_clipping is None else tanh_clipping
    H = policy.decoder.num_heads
    t = decoder_tensors(policy, td)
    B, M, _ = t["emb"].shape
    R, T = actions.shape
    S = max(int(num_starts), 1)
    assert R == S * B
    if multistart is None:
        multistart = S > 1
    env_name = policy.env_name
    filtering = top_k > 0 or 0.0 < top_p < 1.0
    if native is None:
        native = native_reeval_supported(policy, M) and not filtering and not (return_entropy and M > 112)
    if native:
        if filtering:
            raise ValueError("evaluate_log_likelihood: the native re-evaluation kernels do not filter (top_k / top_p)")
        return _evaluate_native(policy, t, td, actions, S, multistart, temperature, clip, rollout_logp, rollout_heads,
                                return_entropy)
    static = {k: td[k] for k in _STATE_KEYS[env_name]}
    # rows are processed in chunks of whole start-groups so that memory stays bounded ([rows, H, T, M] scores)
    starts_per_chunk = max(1, chunk_rows // B)
    bounds = [(s0, min(S, s0 + starts_per_chunk)) for s0 in range(0, S, starts_per_chunk)]
    names = list(t)

    def chunk(c, *tensors):
        s0, s1 = bounds[c]
        out = _logp_rows(env_name, dict(zip(names, tensors)), static, actions[s0 * B:s1 * B], s1 - s0, multistart, H,
                         temperature, clip, top_k, top_p, s_first=s0, return_entropy=return_entropy)
        return torch.cat(out, 1) if return_entropy else out       # (one tensor per chunk: logp | entropy side by side)

    if checkpoint is None:      # ~6 live [rows, H, T, M] fp32 tensors per chunk if the graph is kept
        checkpoint = len(bounds) > 1 and 24.0 * R * H * T * M > 8e9
    if checkpoint and torch.is_grad_enabled():
        res = _ChunkedReeval.apply(chunk, len(bounds), *[t[k] for k in names])
    else:
        res = torch.cat([chunk(c, *[t[k] for k in names]) for c in range(len(bounds))], 0)
    return (res[:, :T], res[:, T:]) if return_entropy else res


def attach_log_likelihood_grad(policy, td, env, actions, native_logp, num_starts: int = 0, multistart=None,
                               temperature=None, tanh_clipping=None):
    """[R, T] per-step log-probs whose VALUE is the native rollout's `native_logp` and whose GRADIENT is the
    re-evaluation's: native + (re - re.detach()).  This is what `AttentionModelPolicy.forward(phase="train")` returns
    under autograd, the counterpart of the reference's graph-attached logprobs (constructive/base.py:236-263)."""
    re = evaluate_log_likelihood(policy, td, env, actions, num_starts=num_starts, multistart=multistart,
                                 temperature=temperature, tanh_clipping=tanh_clipping)
    return native_logp.detach() + (re - re.detach())


_LEGACY_BASELINES = ("shared", "mean", "no", "critic")


def _calculate_loss(baseline, scaler, td, env, out, reward, log_likelihood, extra=None, eam_shapes=False):
    """REINFORCE.calculate_loss (reinforce.py:73-115); eam_shapes: EAM.calculate_loss (earl/model.py:409-457), which first
    reshapes a 1-D baseline value -- concatenated with itself where it has half the rows of `reward`, else unsqueezed and
    expanded to `reward`.  Updates `out` with loss, reinforce_loss, bl_loss, bl_val."""
    bl_val, bl_loss = (extra, 0) if extra is not None else baseline.eval(td, reward, env)
    if eam_shapes and torch.is_tensor(bl_val) and bl_val.dim() == 1:
        if bl_val.shape[0] * 2 == reward.shape[0]:
            bl_val = torch.cat([bl_val, bl_val], dim=0)
        else:
            bl_val = bl_val.unsqueeze(1).expand_as(reward)
    advantage = reward - bl_val
    if scaler is not None:
        advantage = scaler(advantage)
    reinforce_loss = -(advantage * log_likelihood).mean()
    out.update({"loss": reinforce_loss + bl_loss, "reinforce_loss": reinforce_loss, "bl_loss": bl_loss, "bl_val": bl_val})
    return out


def _resolve_baseline(baseline, **kw):
    from .baselines import REINFORCEBaseline, get_reinforce_baseline

    return baseline if isinstance(baseline, REINFORCEBaseline) else get_reinforce_baseline(baseline, **kw)


def _resolve_scaler(reward_scale):
    from .baselines import RewardScaler

    if reward_scale is None or isinstance(reward_scale, RewardScaler):
        return reward_scale
    return RewardScaler(reward_scale)


def reinforce_loss(policy, env, td, baseline: str = "shared", num_starts: int = 0, decode_type: str = None, critic=None,
                   extra=None, reward_scale=None, **rollout_kwargs):
    """One REINFORCE forward as the reference's trainers run it (REINFORCE.shared_step + calculate_loss,
    reinforce.py:59-106; POMO.shared_step, pomo/model.py:89-112): `policy(td, env, phase="train")` under autograd ->
    loss = -((reward - bl) * log_likelihood).mean().

    baseline: "shared" (POMO: mean over the starts of an instance, needs num_starts > 1), "mean" (batch mean), "no", or
    "critic" (CriticBaseline.eval, baselines.py:140-159: v = critic(td).squeeze(-1); the baseline is v.detach() and
    F.mse_loss(v, reward) is added to the loss; `critic`: a critic.CriticNetwork, single rows per instance).
    These four strings keep their own expressions below.  Anything else is a `baselines.REINFORCEBaseline` object or a name of
    `baselines.get_reinforce_baseline` ("exponential", "rollout", "warmup", "rollout_only"; unknown names raise ValueError) and
    runs REINFORCE.calculate_loss as written (reinforce.py:73-115): bl_val, bl_loss = (extra, 0) if `extra` is given -- the
    values `RolloutBaseline.wrap_dataset` stored with the batch -- else baseline.eval(td, reward, env); the advantage passes
    through `reward_scale` (None, an int, "norm" / "scale", or a `baselines.RewardScaler` that keeps its running statistics
    between calls); the output gains reinforce_loss, bl_loss and bl_val.  A baseline with state (exponential, warm-up,
    rollout) must be passed as an object: a name builds a fresh one per call.  With num_starts > 1 reward and
    log-likelihood are [B, S] there, as in POMO.shared_step.
    Returns dict(loss, reward, log_likelihood, actions, ...)."""
    legacy = isinstance(baseline, str) and baseline in _LEGACY_BASELINES and extra is None and reward_scale is None
    if not legacy:
        bl = _resolve_baseline(baseline, **({"critic": critic} if isinstance(baseline, str) and baseline == "critic" else {}))
    elif baseline == "critic":
        if critic is None:
            raise ValueError("reinforce_loss(baseline='critic') needs critic= (critic.create_critic_from_actor(policy))")
        if num_starts > 1:
            raise NotImplementedError("reinforce_loss(baseline='critic') with num_starts > 1 is not built")
    if decode_type is None:
        decode_type = "multistart_sampling" if num_starts > 1 else "sampling"
    kw = dict(rollout_kwargs)
    if num_starts > 1:
        kw["num_starts"] = num_starts
    with torch.enable_grad():
        out = policy(td, env, phase="train", decode_type=decode_type, return_sum_log_likelihood=False, **kw)
    actions, reward, logp = out["actions"], out["reward"], out["log_likelihood"]
    # finished CVRP rows are padded with depot visits of probability 1: their log-prob is 0 and carries no gradient
    ll = logp.sum(1)
    if not legacy:
        out_ = {"reward": reward, "log_likelihood": ll, "actions": actions, "logp_steps": logp, "native_log_likelihood": ll.detach()}
        r, l2 = (unbatchify(reward, num_starts), unbatchify(ll, num_starts)) if num_starts > 1 else (reward, ll)
        with torch.enable_grad():
            return _calculate_loss(bl, _resolve_scaler(reward_scale), td, env, out_, r, l2, extra)
    if baseline == "shared":
        assert num_starts > 1, "shared baseline needs multistart"
        r = unbatchify(reward, num_starts)
        adv = (r - r.mean(1, keepdim=True))
        loss = -(adv * unbatchify(ll, num_starts)).mean()
    elif baseline == "mean":
        loss = -((reward - reward.mean()) * ll).mean()
    elif baseline == "critic":
        with torch.enable_grad():
            v = critic(td).squeeze(-1)
        bl_loss = F.mse_loss(v, reward)
        loss = -((reward - v.detach()) * ll).mean() + bl_loss           # reinforce.py:103-106: reinforce_loss + bl_loss
        return {"loss": loss, "reward": reward, "log_likelihood": ll, "actions": actions, "logp_steps": logp,
                "native_log_likelihood": ll.detach(), "bl_val": v.detach(), "bl_loss": bl_loss}
    else:
        loss = -(reward * ll).mean()
    return {"loss": loss, "reward": reward, "log_likelihood": ll, "actions": actions, "logp_steps": logp,
            "native_log_likelihood": ll.detach()}


def eam_loss(policy, env, td, ea, num_starts: int, improve: bool = True, draws=None, generator=None, return_entropy: bool = True):
    """One EAM training step of the fork with the POMO (shared) baseline (rl4co/models/zoo/earl/model.py:129-247):

    1. sampled multistart rollout, `policy(td, env, phase="train", num_starts=S)` (log-likelihood with grad); with
       return_entropy=True also the entropy of the sampled tours, as the reference's first call asks for (model.py:150-156;
       it only logs it) -- res["entropy"];
    2. the sampled tours are improved by the evolutionary operators on the GPU (`evolution_worker`; the reference
       ships them to CPU threads, model.py:166-171) and get their start column back (`_align_improved_actions`);
    3. the improved tours are evaluated by `policy(td, env, phase="train", actions=improved)` (model.py:189-195);
    4. REINFORCE with the per-instance mean over starts as baseline, over the concatenation [original; improved]
       treated as 2B instances (model.py:226-244, reinforce.py:103-106).

    Returns dict(loss, reward, improved_reward, log_likelihood, improved_log_likelihood, actions, improved_actions)."""
    S = int(num_starts)
    assert S > 1, "the EAM step uses the multistart (shared) baseline"
    with shared_decoder_tensors(policy):        # one differentiable encoder pass for the sampled and the improved tours
        return _eam_loss(policy, env, td, ea, S, improve, draws, generator, return_entropy)


def _eam_loss(policy, env, td, ea, S, improve, draws, generator, return_entropy=False):
    from .evolution import evolution_worker

    with torch.enable_grad():
        out = policy(td, env, phase="train", decode_type="multistart_sampling", num_starts=S, return_entropy=return_entropy)
    actions, reward, ll = out["actions"], out["reward"], out["log_likelihood"]
    rs, lls = [unbatchify(reward, S)], [unbatchify(ll, S)]
    res = {"reward": reward, "log_likelihood": ll, "actions": actions}
    if return_entropy:
        res["entropy"] = out["entropy"]
    if improve:
        with torch.no_grad():
            improved, _ = evolution_worker(actions, td, ea, env, draws=draws, generator=generator)
            if improved.shape[-1] + 1 == actions.shape[-1]:          # _align_improved_actions
                improved = torch.cat([actions[:, :1], improved], dim=-1)
        with torch.enable_grad():
            out2 = policy(td, env, phase="train", actions=improved, num_starts=S, decode_type="multistart_sampling")
        r_imp, ll_imp = out2["reward"], out2["log_likelihood"]
        rs.append(unbatchify(r_imp, S))
        lls.append(unbatchify(ll_imp, S))
        res.update(improved_actions=improved, improved_reward=r_imp, improved_log_likelihood=ll_imp)
    r_all, ll_all = torch.cat(rs, 0), torch.cat(lls, 0)              # [B or 2B, S]
    adv = r_all - r_all.mean(1, keepdim=True)
    res["loss"] = -(adv * ll_all).mean()
    return res


def eam_am_loss(policy, env, td, ea, baseline, extra=None, improve: bool = True, draws=None, generator=None,
                return_entropy: bool = True, reward_scale=None):
    """One EAM training step of the fork with the attention model's baseline, `EAM(baseline="rollout")`
    (rl4co/models/zoo/earl/model.py:150-244 with its calculate_loss, 409-457):

    1. one sampled tour per instance, `policy(td, env, phase="train")` (log-likelihood with grad; return_entropy as in `eam_loss`);
    2. the tours are improved by `evolution_worker` on the GPU (single-start population; an `EA` with method="am");
    3. the improved tours are evaluated by `policy(td, env, phase="train", actions=improved)`, on the encoder graph of step 1;
    4. calculate_loss on the sampled rows [B, 1] and then, with improved tours, on [original; improved] as [2B, 1] rows -- the
       second result is the step's loss.  baseline.eval is therefore called twice in such a step, as in the reference (an
       exponential baseline moves twice); with `extra` (the values `RolloutBaseline.wrap_dataset` stored, [B]) it is not called.

    The shapes are the reference's own: a 1-D `extra` of length B is concatenated to [2B] and subtracted from rewards [2B, 1],
    so the advantage is [2B, 2B] -- row i holds reward_i minus EVERY instance's baseline value -- and the mean over all of
    it makes the effective baseline of a step with `extra` the batch mean of the stored values.
    baseline: a `baselines.REINFORCEBaseline` (e.g. get_reinforce_baseline("rollout") after setup) or a name.
    Returns dict(loss, reinforce_loss, bl_loss, bl_val, reward, log_likelihood, actions[, improved_*][, entropy])."""
    if getattr(policy, "is_ptrnet", False):
        raise NotImplementedError("eam_am_loss: the Pointer Network policy is not built into the EAM step; use reinforce_loss")
    bl, scaler = _resolve_baseline(baseline), _resolve_scaler(reward_scale)
    with shared_decoder_tensors(policy):        # one differentiable encoder pass for the sampled and the improved tours
        return _eam_am_loss(policy, env, td, ea, bl, scaler, extra, improve, draws, generator, return_entropy)


def _eam_am_loss(policy, env, td, ea, bl, scaler, extra, improve, draws, generator, return_entropy):
    from .evolution import evolution_worker

    with torch.enable_grad():
        out = policy(td, env, phase="train", decode_type="sampling", return_entropy=return_entropy)
    actions, reward, ll = out["actions"], out["reward"], out["log_likelihood"]
    res = {"reward": reward, "log_likelihood": ll, "actions": actions}
    if return_entropy:
        res["entropy"] = out["entropy"]
    r0, ll0 = reward[:, None], ll[:, None]                                   # unbatchify(x, (0, 1)): [B, 1]
    with torch.enable_grad():
        _calculate_loss(bl, scaler, td, env, res, r0, ll0, extra, eam_shapes=True)
    if not improve:
        return res
    with torch.no_grad():
        improved, _ = evolution_worker(actions, td, ea, env, draws=draws, generator=generator)
        if improved is not None and improved.shape[-1] + 1 == actions.shape[-1]:          # _align_improved_actions
            improved = torch.cat([actions[:, :1], improved], dim=-1)
        if improved is not None and getattr(env, "name", None) == "op":
            # An empty sampled tour (depot first) is the one parent the OP crossover rebuilds -- into a row that still starts at
            # the depot and then visits customers: not an episode of the env.  Re-evaluated, such a row either raises
            # "infeasible action selected" (seen at OP-20: sampled [0, 0, 0, 0], rebuilt [0, 2, 0, 0]) or comes back with a
            # log-likelihood of -inf, which would make the whole [2B] loss infinite.  Such a row keeps its sampled tour: an
            # unimproved copy.  Only this case is covered: both the sampled and the rebuilt row start at the depot.
            empty = (actions[:, 0] == 0) & (improved[:, 0] == 0)
            improved = torch.where(empty[:, None], actions, improved)
    if improved is None:
        return res
    with torch.enable_grad():
        out2 = policy(td, env, phase="train", actions=improved)
        r_imp, ll_imp = out2["reward"], out2["log_likelihood"]
        res.update(improved_actions=improved, improved_reward=r_imp, improved_log_likelihood=ll_imp)
        r_all, ll_all = torch.cat([r0, r_imp[:, None]], 0), torch.cat([ll0, ll_imp[:, None]], 0)      # [2B, 1]
        td2 = td
        if extra is None:       # combined_td (model.py:234-238): only a baseline evaluated on the fly reads it
            from .tensordict_lite import TensorDict

            td2 = TensorDict({k: torch.cat([v, v], 0) for k, v in td.items() if torch.is_tensor(v)}, batch_size=[2 * td.batch_size[0]])
        _calculate_loss(bl, scaler, td2, env, res, r_all, ll_all, extra, eam_shapes=True)
    return res


def problem_symmetricity_loss(reward, log_likelihood, dim=1):
    """zoo/symnco/losses.py:5-15: REINFORCE with the mean over `dim` as baseline (0 when that axis has fewer than 2 entries)."""
    if reward.shape[dim] < 2:
        return 0
    return (-(reward - reward.mean(dim=dim, keepdim=True)) * log_likelihood).mean()


def solution_symmetricity_loss(reward, log_likelihood, dim=-1):
    """zoo/symnco/losses.py:18-28: the same over the last axis."""
    return problem_symmetricity_loss(reward, log_likelihood, dim)


def invariance_loss(proj_embed, num_augment):
    """zoo/symnco/losses.py:31-39: mean cosine similarity between the projected embeddings of an instance's first copy and its
    other copies -- with the reference's own grouping "(b a) ... -> b a ..." of the rows."""
    pe = proj_embed.reshape(proj_embed.shape[0] // num_augment, num_augment, *proj_embed.shape[1:])
    sim = sum(F.cosine_similarity(pe[:, 0], pe[:, i], dim=-1) for i in range(1, num_augment))
    return sim.mean()


def symeam_loss(policy, env, td, ea, num_augment: int = 4, num_starts: int = 0, alpha: float = 0.2, beta: float = 1.0,
                improve: bool = True, augment=None, draws=None, generator=None):
    """The training branch of `SymEAM.shared_step`, the fork's second trainer (rl4co/models/zoo/earl/model.py:535-660), on a
    `SymNCOPolicy`: symmetric augmentation of the batch (num_augment copies) -> sampled rollout with entropy -> (with
    probability `improve_prob`, decided by the caller: `improve`) evolutionary improvement of the sampled tours and their
    teacher-forced evaluation -> loss = L_ps + beta L_ss + alpha L_inv over [original; improved] (zoo/symnco/losses.py).
    The reference's expressions are kept as written, including which loss is switched by which count (`loss_ps` needs
    num_starts > 1, `loss_ss` num_augment > 1) and the row grouping of the invariance loss.  num_starts > 1: the improved
    tours get their start column back before the evaluation, as in `eam_loss`.
    Returns dict(loss, loss_ps, loss_ss, loss_inv, reward, log_likelihood, actions[, improved_*])."""
    from .evolution import evolution_worker
    from .utils import StateAugmentation

    n_aug, n_start = int(num_augment), int(num_starts)
    if n_aug > 1:
        td = (augment or StateAugmentation(num_augment=n_aug))(td)
    init_td = td.clone()
    kw = dict(num_starts=n_start) if n_start > 1 else {}
    with torch.enable_grad():
        out = policy(td, env, phase="train", return_entropy=True, **kw)
    res = {"reward": out["reward"], "log_likelihood": out["log_likelihood"], "actions": out["actions"], "entropy": out.get("entropy")}
    rs, lls, projs = [unbatchify(out["reward"], (n_aug, n_start))], [unbatchify(out["log_likelihood"], (n_aug, n_start))], \
        [out["proj_embeddings"]]
    if improve:
        with torch.no_grad():
            improved, _ = evolution_worker(out["actions"], init_td, ea, env, draws=draws, generator=generator)
            if improved is not None and improved.shape[-1] + 1 == out["actions"].shape[-1]:
                improved = torch.cat([out["actions"][:, :1], improved], dim=-1)
        if improved is not None:
            with torch.enable_grad():
                out2 = policy(init_td, env, phase="train", actions=improved.to(out["actions"].device), **kw)
            rs.append(unbatchify(out2["reward"], (n_aug, n_start)))
            lls.append(unbatchify(out2["log_likelihood"], (n_aug, n_start)))
            projs.append(out2["proj_embeddings"])
            res.update(improved_actions=improved, improved_reward=out2["reward"], improved_log_likelihood=out2["log_likelihood"])
    reward, ll, proj = torch.cat(rs, 0), torch.cat(lls, 0), torch.cat(projs, 0)
    loss_ps = problem_symmetricity_loss(reward, ll) if n_start > 1 else 0
    loss_ss = solution_symmetricity_loss(reward, ll) if n_aug > 1 else 0
    loss_inv = invariance_loss(proj, n_aug) if n_aug > 1 else 0
    res.update(loss=loss_ps + beta * loss_ss + alpha * loss_inv, loss_ps=loss_ps, loss_ss=loss_ss, loss_inv=loss_inv)
    return res


def polynet_loss(reward, log_likelihood):
    """PolyNet's Poppy loss (zoo/polynet/model.py:195-239 with the shared baseline, rl/reinforce/baselines.py:57-61):
    reward, log_likelihood [B, S]; the baseline is the mean reward of an instance's S rollouts, and only each instance's
    best rollout (the first one among equals in a stable descending order, as the reference's double argsort picks)
    carries gradient.  -> scalar loss = -mean(advantage * log_likelihood * mask) over all B * S entries."""
    bl = reward.mean(dim=1, keepdim=True)
    best = (-reward).argsort(1).argsort(1) < 1
    return -((reward - bl) * log_likelihood * best).mean()


def polynet_step_loss(policy, env, td, num_starts: int, **rollout_kwargs):
    """PolyNet.shared_step in the train phase (zoo/polynet/model.py:124-158): a multisample rollout with `num_starts`
    solutions per instance and `polynet_loss` on it.  Returns the dict `reinforce_loss` returns."""
    with torch.enable_grad():
        out = policy(td, env, phase="train", num_starts=num_starts, multisample=True, return_sum_log_likelihood=False,
                     **rollout_kwargs)
    logp = out["log_likelihood"]
    ll = logp.sum(1)
    loss = polynet_loss(unbatchify(out["reward"], num_starts), unbatchify(ll, num_starts))
    return {"loss": loss, "reward": out["reward"], "log_likelihood": ll, "actions": out["actions"], "logp_steps": logp,
            "native_log_likelihood": ll.detach()}


class PolicyGradientStep:
    """One optimizer step of the reference's REINFORCE / POMO training, data-parallel (BASELINE.json configs[3]):

        out = policy(td, env, phase="train"[, num_starts=S])            # POMO.shared_step, pomo/model.py:89-112
        loss = -((reward - baseline) * log_likelihood).mean()            # reinforce.py:103-106, baselines.py:57-61
        loss.backward() -> ONE flat all-reduce (mean over ranks) -> clip_grad_norm 1.0 -> Adam(lr 1e-4, wd 1e-6)
                                                                         # utils/trainer.py:55,72-89; configs/experiment/routing/pomo.yaml

    Each rank owns its own instances (all starts of an instance on one GPU); the gradient buffer is the only thing
    exchanged (dist.FlatGradBuffer: p.grad are views, no copy kernels around the collective).  At construction every rank
    takes rank 0's parameters and buffers (as DDP does), so the ranks may have been seeded differently; from then on every
    rank ends a step with bit-identical parameters: the reduced buffer is identical on all ranks and the update is
    deterministic.  With batch normalisation in train() mode the running statistics, which each rank updates from its own
    shard, are averaged over the ranks after the step (`sync_buffers`; DDP broadcasts rank 0's instead)."""

    def __init__(self, policy, env, num_starts: int = 0, baseline: str = None, lr: float = 1e-4, weight_decay: float = 1e-6,
                 max_grad_norm: float = 1.0, optimizer=None, baseline_kwargs: dict = None, reward_scale=None):
        from .dist import FlatGradBuffer, broadcast_module_state

        broadcast_module_state(policy, src=0)        # before the optimizer reads the parameters
        self.sync_buffers = any(b.is_floating_point() for b in policy.buffers())
        self.policy, self.env, self.S = policy, env, int(num_starts)
        self.baseline = baseline or ("shared" if self.S > 1 else "mean")
        # "shared" / "mean" / "no" / "critic" stay the strings of `reinforce_loss`; every other value is a baseline object of
        # `baselines` (REINFORCE.__init__, reinforce.py:51-57), with the epoch hooks below
        if not (isinstance(self.baseline, str) and self.baseline in _LEGACY_BASELINES):
            from .baselines import CriticBaseline

            self.baseline = _resolve_baseline(self.baseline, **(baseline_kwargs or {}))
            if isinstance(self.baseline, CriticBaseline) or isinstance(getattr(self.baseline, "baseline", None), CriticBaseline):
                raise NotImplementedError("PolicyGradientStep: a CriticBaseline's parameters are not in this step's gradient buffer "
                                          "or optimizer (use reinforce_loss with your own optimizer, or PPOStep)")
        self.reward_scale = _resolve_scaler(reward_scale)
        self.val_batch_size, self.val_data_size = 64, None
        self.max_grad_norm = max_grad_norm
        self.grads = FlatGradBuffer(policy)
        policy._flat_grads = self.grads
        self.optimizer = optimizer or torch.optim.Adam(policy.parameters(), lr=lr, weight_decay=weight_decay)

    # ---- the epoch hooks of REINFORCE (reinforce.py:117-147); no-ops with the four string baselines --------------------
    def _hooked(self) -> bool:
        return not isinstance(self.baseline, str)

    def _device(self):
        return next(self.policy.parameters()).device

    def setup(self, batch_size: int = 64, dataset_size: int = None):
        """post_setup_hook: baseline.setup(policy, env, batch_size=val_batch_size, device, dataset_size=val_data_size).
        dataset_size is the size of the rollout baseline's evaluation dataset: required (at least 2) with "rollout" /
        "rollout_only", where its absence raises ValueError here; unused by the other baselines."""
        self.val_batch_size, self.val_data_size = int(batch_size), dataset_size
        if self._hooked():
            self.baseline.setup(self.policy, self.env, batch_size=self.val_batch_size, device=self._device(),
                                dataset_size=dataset_size)

    def wrap_dataset(self, dataset):
        """The epoch's training dataset as the baseline wants it (the rollout baseline adds its values under "extra")."""
        if not self._hooked():
            return dataset
        return self.baseline.wrap_dataset(dataset, self.env, batch_size=self.val_batch_size, device=self._device())

    def on_epoch_end(self, epoch: int):
        """on_train_epoch_end: the baseline's epoch_callback (the rollout baseline's challenge, the warm-up's alpha)."""
        if self._hooked():
            self.baseline.epoch_callback(self.policy, env=self.env, batch_size=self.val_batch_size, device=self._device(),
                                         epoch=epoch, dataset_size=self.val_data_size)

    def __call__(self, td, extra=None, **rollout_kwargs) -> dict:
        self.grads.zero_()
        if getattr(self.policy.decoder, "is_polynet", False):       # PolyNet trains on its Poppy loss (num_starts = k in the reference)
            out = polynet_step_loss(self.policy, self.env, td, self.S, **rollout_kwargs)
        else:       # (one of the four strings without extra / reward_scale: reinforce_loss's own expressions, as before)
            out = reinforce_loss(self.policy, self.env, td, baseline=self.baseline, num_starts=self.S, extra=extra,
                                 reward_scale=self.reward_scale, **rollout_kwargs)
        out["loss"].backward()
        if not self.grads.attached():
            raise RuntimeError("PolicyGradientStep: p.grad is no longer a view of the flat buffer (zero_grad(set_to_none)?)")
        self.grads.allreduce(average=True)
        out["grad_norm"] = self.grads.clip_(self.max_grad_norm) if self.max_grad_norm else None
        self.optimizer.step()
        if self.sync_buffers and self.policy.training:
            from .dist import allreduce_buffers

            allreduce_buffers(self.policy)
        return out


def fit(step, env, epochs: int, train_data_size: int, batch_size: int, val_data_size: int, val_batch_size: int = None,
        lr_milestones=None, lr_gamma: float = 0.1, on_step=None) -> list:
    """The reference's training loop around a `PolicyGradientStep`, as a plain loop (RL4COLitModule's setup / train
    dataloader regenerated per epoch / on_train_epoch_end, rl/common/base.py; REINFORCE's hooks, reinforce.py:117-147):

        step.setup(val_batch_size, val_data_size)       # val_data_size: required by the rollout baseline (>= 2 instances)
        per epoch:  data = step.wrap_dataset(env.dataset([train_data_size]) as one TensorDict on the policy's device)
                    per batch, in order (the data is fresh every epoch: no shuffle):  step(env.reset(batch), extra=batch["extra"] if any)
                    step.on_epoch_end(epoch);  MultiStepLR(lr_milestones, lr_gamma).step() if milestones are given

    The dataset never leaves the device; an epoch's mean loss and reward are read once, at its end.  on_step(epoch, i, out):
    optional callback.  -> one dict per epoch: epoch, loss, reward, steps[, alpha][, baseline_mean]."""
    from .baselines import as_tensordict

    device = next(step.policy.parameters()).device
    step.setup(batch_size=val_batch_size or batch_size, dataset_size=val_data_size)
    sched = None
    if lr_milestones:
        sched = torch.optim.lr_scheduler.MultiStepLR(step.optimizer, milestones=list(lr_milestones), gamma=lr_gamma)
    history = []
    for epoch in range(int(epochs)):
        data = step.wrap_dataset(as_tensordict(env.dataset([train_data_size]), device))
        data = as_tensordict(data, device)
        n = data.batch_size[0]
        losses, rewards = [], []
        for bi, i in enumerate(range(0, n, batch_size)):
            batch = data[i:i + batch_size]
            out = step(env.reset(batch), extra=batch.get("extra", None))
            losses.append(out["loss"].detach())
            rewards.append(out["reward"].detach().mean())
            if on_step is not None:
                on_step(epoch, bi, out)
        step.on_epoch_end(epoch)
        if sched is not None:
            sched.step()
        rec = {"epoch": epoch, "steps": len(losses), "loss": float(torch.stack(losses).mean()),
               "reward": float(torch.stack(rewards).mean())}
        bl = step.baseline
        if hasattr(bl, "alpha"):
            rec["alpha"] = float(bl.alpha)
        inner = getattr(bl, "baseline", bl)
        if hasattr(inner, "mean") and not callable(inner.mean):
            rec["baseline_mean"] = float(inner.mean)
        history.append(rec)
    return history


# ------------------------------------------------------------------------------------------------------------
# PPO (rl4co/models/rl/ppo/ppo.py:61-235, rl4co/models/zoo/amppo/model.py)
# ------------------------------------------------------------------------------------------------------------
def ppo_loss_terms(ll_new, ll_old, reward, value, entropy, clip_range: float = 0.2, vf_lambda: float = 0.5,
                   entropy_lambda: float = 0.0, normalize_adv: bool = False) -> dict:
    """The loss of one PPO mini-batch, ppo.py:177-209 line by line.  ll_new [b] (summed log-likelihood under the current
    policy, with a graph), ll_old [b] (the rollout's), reward [b] or [b, 1], value [b, 1] (the critic's, with a graph),
    entropy [b].  -> dict(loss, surrogate_loss, value_loss, entropy = entropy.mean())."""
    previous_reward = reward.view(-1, 1)
    ratio = torch.exp(ll_new - ll_old).view(-1, 1)                      # [batch, 1]
    adv = previous_reward - value.detach()
    if normalize_adv:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    surrogate_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip_range, 1 + clip_range) * adv).mean()
    value_loss = F.huber_loss(value, previous_reward)
    ent = entropy.mean()
    loss = surrogate_loss + vf_lambda * value_loss - entropy_lambda * ent
    return {"loss": loss, "surrogate_loss": surrogate_loss, "value_loss": value_loss, "entropy": ent}


def _ppo_mini_batch_size(mini_batch_size):
    """The constructor's rules and warnings of ppo.py:87-101."""
    import logging

    log = logging.getLogger(__name__)
    if isinstance(mini_batch_size, bool) or not isinstance(mini_batch_size, (int, float)):
        raise ValueError("mini_batch_size must be an integer or a float.")
    if isinstance(mini_batch_size, float) and (mini_batch_size <= 0 or mini_batch_size > 1):
        log.warning("mini_batch_size must be an integer or a float in the range (0, 1], got %s. Setting mini_batch_size to %s.",
                    mini_batch_size, 0.25)
        mini_batch_size = 0.25
    if isinstance(mini_batch_size, int) and mini_batch_size <= 0:
        log.warning("mini_batch_size must be an integer or a float in the range (0, 1], got %s. Setting mini_batch_size to %s.",
                    mini_batch_size, 128)
        mini_batch_size = 128
    return mini_batch_size


def _ppo_resolve_mini_batch(mini_batch_size, batch_size: int) -> int:
    """ppo.py:139-148: a float is a fraction of the batch, the size is capped at the batch."""
    mb = int(batch_size * mini_batch_size) if isinstance(mini_batch_size, float) else int(mini_batch_size)
    if mb <= 0:
        raise ValueError(f"mini_batch_size={mini_batch_size!r} of a batch of {batch_size} is an empty mini-batch")
    return min(mb, batch_size)


class PPOStep:
    """One training step of the reference's PPO (ppo.py:128-232; AMPPO, zoo/amppo/model.py, is this with the attention model):

        no_grad: out = policy(td.clone(), env, phase="train")           -> actions, reward, old log-likelihood
        ppo_epochs x shuffled mini-batches (the last partial one kept, as a DataLoader without drop_last):
            out = policy(sub.clone(), env, phase="train", actions=A[idx], return_entropy=True, return_sum_log_likelihood=False)
            value = critic(sub);  ppo_loss_terms;  zero grads, backward, ONE flat all-reduce over policy + critic gradients
            (mean over the ranks), clip the global norm to max_grad_norm, optimizer.step()

    The tours are fixed after the rollout, so every mini-batch pass is the teacher-forced re-evaluation: log-likelihood AND
    entropy come with a graph from the native kernels where they serve the env and size (eamrl_reeval_forward / _backward with
    eamrl_reeval.gent), from the PyTorch expression otherwise (PDP, graphs above 112 nodes).  Depot-padded columns of the
    action rows are steps with one feasible node: log-prob 0, entropy 0, no gradient.
    Defaults are the reference's (ppo.py:61-111).  A PolyNet policy has no re-evaluation with given actions on this path."""

    def __init__(self, policy, env, critic=None, clip_range: float = 0.2, ppo_epochs: int = 2, mini_batch_size=0.25,
                 vf_lambda: float = 0.5, entropy_lambda: float = 0.0, normalize_adv: bool = False, max_grad_norm: float = 0.5,
                 lr: float = 1e-4, optimizer=None, generator=None):
        from .critic import create_critic_from_actor
        from .dist import FlatGradBuffer, broadcast_module_state

        if getattr(policy, "is_ptrnet", False):
            raise NotImplementedError("PPOStep: the Pointer Network policy is not built into PPO (no critic from its encoder, no "
                                      "entropy); train it with reinforce_loss / PolicyGradientStep")
        if getattr(policy.decoder, "is_polynet", False):
            raise NotImplementedError("PPOStep: a PolyNet policy has no re-evaluation with given actions (actions=) on this path")
        if critic is None:
            critic = create_critic_from_actor(policy)
        self.policy, self.env, self.critic = policy, env, critic
        self.clip_range, self.ppo_epochs = float(clip_range), int(ppo_epochs)
        self.mini_batch_size = _ppo_mini_batch_size(mini_batch_size)
        self.vf_lambda, self.entropy_lambda, self.normalize_adv = float(vf_lambda), float(entropy_lambda), bool(normalize_adv)
        self.max_grad_norm = max_grad_norm
        self.generator = generator
        self.modules = nn.ModuleList([policy, critic])
        broadcast_module_state(self.modules, src=0)          # before the optimizer reads the parameters
        self.grads = FlatGradBuffer(self.modules)
        self.optimizer = optimizer or torch.optim.Adam(self.modules.parameters(), lr=lr)

    def partition(self, batch_size: int):
        """One epoch's mini-batches: a permutation of the batch cut into consecutive pieces -> list of index tensors (CPU)."""
        mb = _ppo_resolve_mini_batch(self.mini_batch_size, batch_size)
        perm = torch.randperm(batch_size, generator=self.generator)
        return [perm[i:i + mb] for i in range(0, batch_size, mb)]

    def mini_batch_terms(self, sub, actions, ll_old, reward) -> dict:
        """ppo.py:168-209 on one mini-batch: -> ppo_loss_terms(...) plus ll [b, T], entropy [b] and value [b, 1] (graphs attached)."""
        with torch.enable_grad():
            out = self.policy(sub.clone(), self.env, phase="train", actions=actions, return_entropy=True,
                              return_sum_log_likelihood=False)
            ll, entropy = out["log_likelihood"], out["entropy"]
            value = self.critic(sub)
            terms = ppo_loss_terms(ll.sum(dim=-1), ll_old, reward, value, entropy, self.clip_range, self.vf_lambda,
                                   self.entropy_lambda, self.normalize_adv)
        terms.update(ll=ll, entropy_rows=entropy, value=value)
        return terms

    def __call__(self, td) -> dict:
        with torch.no_grad():
            out = self.policy(td.clone(), self.env, phase="train")
        actions, reward, ll_old = out["actions"], out["reward"], out["log_likelihood"]
        B = actions.shape[0]
        steps, terms = 0, None
        for _ in range(self.ppo_epochs):
            for idx in self.partition(B):
                sub = td[idx]                       # (sub_td of the reference's DataLoader: the rows of the instance tensors)
                idx = idx.to(actions.device)
                terms = self.mini_batch_terms(sub, actions[idx].contiguous(), ll_old[idx], reward[idx])
                self.grads.zero_()
                terms["loss"].backward()
                if not self.grads.attached():
                    raise RuntimeError("PPOStep: p.grad is no longer a view of the flat buffer (zero_grad(set_to_none)?)")
                self.grads.allreduce(average=True)
                if self.max_grad_norm is not None:
                    self.grads.clip_(self.max_grad_norm)
                self.optimizer.step()
                steps += 1
        return {"loss": terms["loss"].detach(), "surrogate_loss": terms["surrogate_loss"].detach(),
                "value_loss": terms["value_loss"].detach(), "entropy": terms["entropy"].detach(), "reward": reward,
                "actions": actions, "optimizer_steps": steps}
