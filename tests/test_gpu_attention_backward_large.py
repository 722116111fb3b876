"""GPU: the encoder self-attention backward for graphs of 113 to 1024 nodes (k_mha_encoder_bwd_mfma behind
eamrl_mha_encoder_backward), and what it gives the training graph there: no torch attention, and for instance-norm
policies one encoder pass per training step."""
import os

import pytest
import torch
import torch.nn.functional as F

from test_gpu_parity import DEV, assert_bits_equal

pytestmark = pytest.mark.gpu


def _qkv(B, N, seed, amp=1.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = (torch.randn(B, N, 384, generator=g) * amp).to(DEV)
    dout = torch.randn(B, N, 128, generator=g).to(DEV)
    return qkv, dout


@pytest.mark.parametrize("B,N,amp", [(2, 113, 1.5), (1, 128, 1.5), (3, 200, 1.5), (2, 257, 1.5), (1, 501, 1.5), (2, 512, 1.5),
                                     (1, 1000, 1.5), (1, 1024, 1.5), (2, 300, 6.0), (1, 1024, 6.0)])
def test_large_graph_attention_backward_matches_float64_autograd(B, N, amp):
    """ops.mha_encoder_backward above 112 nodes against autograd through scaled_dot_product_attention in float64 on the same
    packed qkv, with the tolerances of the <= 112-node kernel's test.  amp 6.0 (qkv x 4) gives peaked softmax rows: scores of
    some hundreds, whose fp32 rounding alone moves the weights by more than those bounds; there each bound is the larger of
    the base one and twice the error of torch's own fp32 SDPA (forward and backward) on the same input."""
    from eam_rl4co_amd import ops

    qkv, dout = _qkv(B, N, B * 131 + N, amp)
    y = ops.mha_encoder(qkv, 8)
    dqkv = ops.mha_encoder_backward(qkv, dout, 8)

    def sdpa(x):
        x = x.requires_grad_()
        q = x.view(B, N, 3, 8, 16).permute(2, 0, 3, 1, 4)
        out = F.scaled_dot_product_attention(q[0], q[1], q[2]).permute(0, 2, 1, 3).reshape(B, N, 128)
        (out * dout.to(out.dtype)).sum().backward()
        return out.detach().double(), x.grad.double()

    ref, dref = sdpa(qkv.double())
    tol_y, tol_g = 2e-6 * float(ref.abs().max()), 1e-5 * float(dref.abs().max())
    if amp > 1.5:
        y32, d32 = sdpa(qkv.clone())
        tol_y = max(tol_y, 2 * float((y32 - ref).abs().max()))
        tol_g = max(tol_g, 2 * float((d32 - dref).abs().max()))
    err_y = float((y.double() - ref).abs().max())
    err_g = float((dqkv.double() - dref).abs().max())
    assert err_y <= tol_y, (err_y, tol_y)
    assert err_g <= tol_g, (err_g, tol_g)


@pytest.mark.parametrize("N", [150, 501, 1024])
def test_large_graph_attention_backward_is_deterministic_and_batch_independent(N):
    from eam_rl4co_amd import ops

    qkv, dout = _qkv(4, N, N)
    a = ops.mha_encoder_backward(qkv, dout, 8)
    b = ops.mha_encoder_backward(qkv, dout, 8)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    one = ops.mha_encoder_backward(qkv[:1].contiguous(), dout[:1].contiguous(), 8)
    assert torch.equal(one[0].view(torch.int32), a[0].view(torch.int32))


def test_attention_backward_covers_graphs_up_to_1024_nodes():
    from eam_rl4co_amd import ops

    assert all(ops.mha_encoder_backward_supported(n, 128, 8) for n in range(1, 1025))
    assert not ops.mha_encoder_backward_supported(1025, 128, 8)
    assert not ops.mha_encoder_backward_supported(200, 64, 8) and not ops.mha_encoder_backward_supported(200, 128, 4)
    qkv, dout = _qkv(1, 1025, 0)
    with pytest.raises(RuntimeError, match="eamrl_mha_encoder_backward"):
        ops.mha_encoder_backward(qkv, dout, 8)


def _policy(env_name, norm, seed=0):
    import eam_rl4co_amd as ea

    torch.manual_seed(seed)
    return ea.AttentionModelPolicy(env_name=env_name, normalization=norm).to(DEV).train()


@pytest.mark.parametrize("env_name,N", [("cvrp", 200), ("tsp", 150)])
@pytest.mark.parametrize("norm", ["batch", "instance"])
def test_large_graph_training_step_runs_without_torch_attention(env_name, N, norm, monkeypatch):
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import train

    def no_sdpa(*a, **k):
        raise AssertionError("scaled_dot_product_attention called")

    env = ea.get_env(env_name, generator_params=dict(num_loc=N), seed=N)
    torch.manual_seed(N)
    td = env.reset(batch_size=[4]).to(DEV)
    pol = _policy(env_name, norm)
    monkeypatch.setattr(F, "scaled_dot_product_attention", no_sdpa)
    monkeypatch.setattr(torch.nn.functional, "scaled_dot_product_attention", no_sdpa)
    out = train.reinforce_loss(pol, env, td, baseline="mean")
    out["loss"].backward()
    grads = [p.grad for p in pol.encoder.parameters() if p.requires_grad]
    assert grads and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)


@pytest.mark.parametrize("env_name,N,B", [("tsp", 150, 4), ("cvrp", 230, 3), ("cvrp", 501, 2)])
def test_large_graph_training_encoder_equals_native_encoder(env_name, N, B):
    """As test_training_graph_encoder_equals_native_encoder above 112 nodes: the training graph's encoder reproduces the
    native encoder bit for bit, so instance-norm policies take one encoder pass per step there too."""
    import eam_rl4co_amd as ea
    from eam_rl4co_amd.train import encode_autograd, graph_encoder_equals_native

    env = ea.get_env(env_name, generator_params=dict(num_loc=N), seed=N)
    torch.manual_seed(N + B)
    td = env.reset(batch_size=[B]).to(DEV)
    assert td["locs"].shape[1] > 112
    pol = _policy(env_name, "instance", seed=N)
    assert graph_encoder_equals_native(pol, td)
    with torch.no_grad():
        native, _ = pol.encoder(td)
    graph = encode_autograd(pol, td)
    assert graph.requires_grad
    assert_bits_equal(graph.detach(), native.cpu().numpy(), "embeddings")
    res = []
    for separate in ("0", "1"):
        os.environ["EAMRL_SEPARATE_ENCODER_PASSES"] = separate
        try:
            torch.manual_seed(5)
            out = pol(td.clone(), env, phase="train", decode_type="sampling")
        finally:
            os.environ.pop("EAMRL_SEPARATE_ENCODER_PASSES", None)
        assert out["log_likelihood"].requires_grad
        res.append(out)
    assert torch.equal(res[0]["actions"], res[1]["actions"]) and torch.equal(res[0]["reward"], res[1]["reward"])
    assert torch.equal(res[0]["log_likelihood"].detach(), res[1]["log_likelihood"].detach())


@pytest.mark.parametrize("env_name,N,B,norm", [("cvrp", 230, 4, "batch"), ("cvrp", 230, 4, "instance"), ("tsp", 500, 2, "instance")])
def test_large_graph_training_gradients_match_torch_attention(env_name, N, B, norm, monkeypatch):
    """A whole training step with the native attention backward against the same step with torch's attention
    (EAMRL_TORCH_ATTENTION=1): every parameter gradient within 1e-4 norm-wise, with the absolute floor of the other training
    tests (gradients that are rounding noise are measured against the largest gradient norm).  Where a gradient is a sum
    that cancels (TSP-500: init_embed.weight, norm 318 against 2282 for the largest) two fp32 attentions differ by more than
    that; such a gradient is measured against a third run with the graph's attention in float64, and the native one must
    be at least as close to it as twice torch's fp32 one."""
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import train

    env = ea.get_env(env_name, generator_params=dict(num_loc=N), seed=N)
    torch.manual_seed(N + B)
    td = env.reset(batch_size=[B]).to(DEV)
    pol = _policy(env_name, norm, seed=N)
    M = td["locs"].shape[1]
    g = torch.Generator().manual_seed(3)
    noise = torch.empty(B, 2 * M + 1, M).exponential_(1, generator=g).to(DEV)

    def attention64(qkv, B, N, E, H):
        q = qkv.double().view(B, N, 3, H, E // H).permute(2, 0, 3, 1, 4)
        return F.scaled_dot_product_attention(q[0], q[1], q[2]).permute(0, 2, 1, 3).reshape(B, N, E).float()

    grads, acts = [], []
    for run in ("native", "torch", "float64"):
        monkeypatch.setenv("EAMRL_TORCH_ATTENTION", "0" if run == "native" else "1")
        if run == "float64":        # (the rollout keeps the native encoder: EAMRL_TORCH_ATTENTION=1 means two encoder passes)
            monkeypatch.setattr(train, "_self_attention", attention64)
        for p in pol.parameters():
            p.grad = None
        out = train.reinforce_loss(pol, env, td.clone(), baseline="mean", noise=noise)
        out["loss"].backward()
        acts.append(out["actions"])
        grads.append({k: (p.grad.clone() if p.grad is not None else None) for k, p in pol.named_parameters()})
    assert torch.equal(acts[0], acts[1]) and torch.equal(acts[0], acts[2])
    top = max(float(g.norm()) for g in grads[1].values() if g is not None)
    for k in grads[0]:
        a, r, r64 = grads[0][k], grads[1][k], grads[2][k]
        assert (a is None) == (r is None), k
        if a is not None:
            if float((a - r).norm()) <= 1e-4 * float(r.norm()) + 1e-5 * top:
                continue
            err, err32 = float((a - r64).norm()), float((r - r64).norm())
            assert err <= max(1e-4 * float(r64.norm()) + 1e-5 * top, 2 * err32), (k, err, err32, float(r64.norm()))
