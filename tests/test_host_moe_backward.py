"""CPU (no GPU needed): the native backward of the MoE sublayer's experts -- the C ABI surface of eamrl_moe_experts_forward /
_backward (declared, exported, bound; every bad argument refused before a launch; the scratch formulas), the `ops` wrappers'
refusal off the GPU, the choice between `train.moe_autograd` and `train.moe_autograd_native`, and tests/moe_grad_ref.py (the
float64 statement the GPU tests measure against) against torch.autograd through `train.moe_autograd`.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import moe_grad_ref
import moe_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eamrl_moe_experts_forward_scratch", "eamrl_moe_experts_backward_scratch", "eamrl_moe_experts_forward",
       "eamrl_moe_experts_backward")


def test_entry_points_are_declared_exported_and_bound():
    from eam_rl4co_amd import _lib

    with open(os.path.join(ROOT, "include", "eamrl.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/eamrl.h"
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name) is not None
    assert "typedef struct eamrl_moe_experts" in text
    # the binding mirrors the struct field for field
    body = re.search(r"typedef struct eamrl_moe_experts \{(.*?)\} eamrl_moe_experts;", text, flags=re.S).group(1)
    fields = [re.search(r"([A-Za-z_0-9]+)\s*$", part).group(1) for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert fields == [n for n, _ in _lib.MoeExperts._fields_], fields


def nch(rows, n, k):
    return max(1, min(128 // n, -(-(rows * k) // 64)))


def test_scratch_queries_match_the_documented_formulas():
    from eam_rl4co_amd import _lib, ops

    lib = _lib.load()
    for rows in (0, 1, 15, 16, 17, 255, 256, 257, 16 * 37 + 5, 51712, 1 << 24):
        for n, k in ((4, 2), (4, 1), (4, 4), (2, 1), (8, 2), (1, 1), (8, 8), (3, 2)):
            state = 64 + 16 * ((rows * n + 3) // 4) + 512 * rows * k + 16 * ((rows * k + 15) // 16) + 32 * ((rows + 255) // 256)
            assert lib.eamrl_moe_experts_forward_scratch(rows, n, k) == state == ops.moe_experts_forward_scratch(rows, n, k), (rows, n, k)
            bwd = 5632 * rows * k + 264192 * n * nch(rows, n, k)
            assert lib.eamrl_moe_experts_backward_scratch(rows, n, k) == bwd == ops.moe_experts_backward_scratch(rows, n, k), (rows, n, k)
    for rows, n, k in ((-1, 4, 2), ((1 << 24) + 1, 4, 2), (16, 9, 2), (16, 0, 0), (16, 4, 0), (16, 4, 5)):
        assert lib.eamrl_moe_experts_forward_scratch(rows, n, k) == -1, (rows, n, k)
        assert lib.eamrl_moe_experts_backward_scratch(rows, n, k) == -1, (rows, n, k)


FWD_PTRS = ("x", "sel", "g", "W1p", "b1", "W2p", "b2", "y", "state")
BWD_PTRS = ("x", "g", "W1p", "b1", "W1Tp", "W2Tp", "dy", "state", "scratch")
BWD_OUT = ("dx", "dg", "dW1", "db1", "dW2", "db2")


def test_abi_refuses_bad_arguments_before_a_launch():
    """Every call below is rejected by the argument checks (return -1, eamrl_last_error names the entry point), so none reaches
    a launch: the pointers are dummies."""
    from eam_rl4co_amd import _lib

    lib = _lib.load()
    big = 1 << 40

    def args(ptrs, **over):
        m = _lib.MoeExperts()
        for name in ptrs:
            setattr(m, name, 0x1000)
        m.rows, m.embed_dim, m.hidden, m.n_exp, m.k, m.state_bytes, m.scratch_bytes = 16, 128, 512, 4, 2, big, big
        for key, v in over.items():
            setattr(m, key, v)
        return m

    shape_cases = [dict(embed_dim=64), dict(hidden=256), dict(n_exp=9), dict(n_exp=0, k=0), dict(k=0), dict(k=5), dict(rows=-1),
                   dict(rows=(1 << 24) + 1)]
    fwd = ([args(FWD_PTRS, **c) for c in shape_cases] + [args(FWD_PTRS, **{p: None}) for p in FWD_PTRS]
           + [args(FWD_PTRS, state_bytes=lib.eamrl_moe_experts_forward_scratch(16, 4, 2) - 1), args(FWD_PTRS, state_bytes=0)]
           + [args(FWD_PTRS, **{p: 0x1004}) for p in ("x", "W1p", "W2p", "b2", "y", "state")])
    assert lib.eamrl_moe_experts_forward(None, None) == -1 and b"eamrl_moe_experts_forward" in lib.eamrl_last_error()
    for i, m in enumerate(fwd):
        assert lib.eamrl_moe_experts_forward(C.byref(m), None) == -1, i
        assert b"eamrl_moe_experts_forward: requirement failed" in lib.eamrl_last_error(), i
    assert lib.eamrl_moe_experts_forward(C.byref(args(FWD_PTRS, rows=0)), None) == 0           # an empty batch: nothing to launch

    all_bwd = BWD_PTRS + BWD_OUT
    bwd = ([args(all_bwd, **c) for c in shape_cases] + [args(all_bwd, **{p: None}) for p in BWD_PTRS]
           + [args(all_bwd, **{p: None}) for p in ("dW1", "db1", "dW2", "db2")]             # the weight gradients: all or none
           + [args(BWD_PTRS + ("dx", "dg", "db2"))]
           + [args(all_bwd, state_bytes=lib.eamrl_moe_experts_forward_scratch(16, 4, 2) - 1),
              args(all_bwd, scratch_bytes=lib.eamrl_moe_experts_backward_scratch(16, 4, 2) - 1), args(all_bwd, scratch_bytes=0)]
           + [args(all_bwd, **{p: 0x1004}) for p in ("x", "W1p", "W1Tp", "W2Tp", "dy", "dx", "dW1", "db1", "dW2", "db2", "state",
                                                     "scratch")])
    assert lib.eamrl_moe_experts_backward(None, None) == -1 and b"eamrl_moe_experts_backward" in lib.eamrl_last_error()
    for i, m in enumerate(bwd):
        assert lib.eamrl_moe_experts_backward(C.byref(m), None) == -1, i
        assert b"eamrl_moe_experts_backward: requirement failed" in lib.eamrl_last_error(), i
    assert lib.eamrl_moe_experts_backward(C.byref(args(all_bwd, rows=0)), None) == 0


def test_no_cpu_fallback():
    from eam_rl4co_amd import ops, train

    x, g, sel = torch.zeros(4, 128), torch.full((4, 2), 0.5), torch.zeros(4, 2, dtype=torch.int8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.moe_experts_forward(x, sel, g, {})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.moe_experts_backward(x, x, g, {}, torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pack_moe_experts_backward([torch.zeros(512, 128)], [torch.zeros(128, 512)])
    params = [torch.zeros(s, requires_grad=True) for s in ((512, 128), (512,), (128, 512), (128,))]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train._MoEExpertsFn.apply(x, g[:, :1], sel[:, :1], None, *params)


def make_module(dtype=torch.float32, **over):
    from eam_rl4co_amd.policy import MoE

    torch.manual_seed(11)
    m = MoE(128, 128, num_neurons=[512], **dict(moe_ref.MOE_KWARGS["encoder"], **over)).train()
    with torch.no_grad():
        m.w_gate.normal_(0, 0.3)
        m.w_noise.normal_(0, 0.1)
    return m.to(dtype)


def test_cpu_input_and_the_switch_choose_the_torch_expression(monkeypatch):
    """`encode_autograd` asks `moe_native_backward`: CPU tensors keep `moe_autograd`, and so does EAMRL_MOE_NATIVE_BACKWARD=0
    whatever the device (the question is answered on attributes only, so a stand-in tensor serves for the GPU)."""
    from eam_rl4co_amd import train

    m = make_module()
    h = torch.randn(2, 5, 128)
    monkeypatch.delenv("EAMRL_MOE_NATIVE_BACKWARD", raising=False)
    assert not train.moe_native_backward(m, h)
    assert not train.moe_native_backward(m, h.double())

    class OnGpu:
        is_cuda, dtype = True, torch.float32

    class Mod:
        w_gate = OnGpu()

    assert train.moe_native_backward(Mod(), OnGpu())
    monkeypatch.setenv("EAMRL_MOE_NATIVE_BACKWARD", "0")
    assert not train.moe_native_backward(Mod(), OnGpu())
    monkeypatch.setenv("EAMRL_MOE_NATIVE_BACKWARD", "1")
    assert train.moe_native_backward(Mod(), OnGpu())
    # and what encode_autograd then calls on CPU tensors is moe_autograd itself
    calls = []
    orig = train.moe_autograd
    monkeypatch.setattr(train, "moe_autograd", lambda *a: calls.append(1) or orig(*a))
    monkeypatch.setattr(train, "moe_autograd_native", lambda *a: pytest.fail("the native path was chosen for CPU tensors"))
    import eam_rl4co_amd as ea

    pol = ea.AttentionModelPolicy(env_name="tsp", moe_kwargs=moe_ref.MOE_KWARGS).eval()
    env = ea.get_env("tsp", generator_params=dict(num_loc=6), seed=1)
    monkeypatch.setenv("EAMRL_TORCH_LINEAR", "1")
    emb = train.encode_autograd(pol, env.reset(batch_size=[2]))
    assert emb.shape == (2, 6, 128) and len(calls) == 3


@pytest.mark.parametrize("n_exp,k", [(4, 2), (3, 1), (2, 2)])
def test_grad_ref_agrees_with_autograd_through_moe_autograd(n_exp, k):
    """float64 on the CPU: the hand-written formula against torch.autograd through the all-torch expression.  The routing the
    reference function takes is read back from the gate of `moe_autograd` (recomputed here with the same expression)."""
    from eam_rl4co_amd import train

    m = make_module(torch.float64, num_experts=n_exp, k=k, noisy_gating=False)
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((37, 128))).requires_grad_(True)
    dy = torch.from_numpy(rng.standard_normal((37, 128)))
    y = train.moe_autograd(m, x, True)
    y.backward(dy)
    with torch.no_grad():
        p = torch.softmax(x @ m.w_gate, -1)
        top_p, top_i = torch.sort(p, dim=-1, descending=True, stable=True)
        top_p, top_i = top_p[:, :k], top_i[:, :k]
        g = top_p / (top_p.sum(1, keepdim=True) + 1e-6)
    W1, b1, W2, b2 = (np.stack([getattr(ex.lins[i], nm).detach().numpy() for ex in m.experts])
                      for i, nm in ((0, "weight"), (0, "bias"), (1, "weight"), (1, "bias")))
    ref = moe_grad_ref.experts_grad_ref(x.detach().numpy(), top_i.numpy(), g.numpy(), W1, b1, W2, b2, dy.numpy())
    np.testing.assert_allclose(ref["y"], y.detach().numpy(), rtol=0, atol=1e-12)
    for e, ex in enumerate(m.experts):
        for key, par in (("dW1", ex.lins[0].weight), ("db1", ex.lins[0].bias), ("dW2", ex.lins[1].weight), ("db2", ex.lins[1].bias)):
            np.testing.assert_allclose(ref[key][e], par.grad.numpy(), rtol=0, atol=1e-11, err_msg=f"{key}[{e}]")
    # dx of the expression also flows through the gate: take that part off with dg of the reference
    xg = x.detach().clone().requires_grad_(True)
    pg = torch.softmax(xg @ m.w_gate.detach(), -1)
    tp = torch.gather(pg, 1, top_i)
    (tp / (tp.sum(1, keepdim=True) + 1e-6)).backward(torch.from_numpy(ref["dg"]))
    np.testing.assert_allclose(ref["dx"] + xg.grad.numpy(), x.grad.numpy(), rtol=0, atol=1e-11)


def test_grad_ref_cases_have_the_routings_they_name():
    c = moe_grad_ref.make_case(98, 4, 1, 3, routing=(1, 16, 17, 64))
    assert np.bincount(c["sel"].reshape(-1), minlength=4).tolist() == [1, 16, 17, 64]
    c = moe_grad_ref.make_case(65, 4, 2, 3, routing="skip_last")
    assert np.bincount(c["sel"].reshape(-1), minlength=4)[3] == 0
    c = moe_grad_ref.make_case(65, 4, 2, 3, routing="all_on_0")
    assert np.bincount(c["sel"].reshape(-1), minlength=4)[0] == 65
    assert all(len(set(r.tolist())) == 2 for r in c["sel"])
    ref = moe_grad_ref.experts_grad_ref(**moe_grad_ref.make_case(5, 4, 2, 3, routing="skip_last"))
    assert not ref["dW1"][3].any() and not ref["db2"][3].any() and ref["dW1"][0].any()
