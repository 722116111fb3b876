"""GPU: every kernel instantiation behind ops.linear / ops.matmul_right against the oracle, bit for bit, on the operand layouts of
tests/linear_cases.py: windows of wider buffers, misaligned bases, planes of a slot-major buffer.  The whole output buffer is
compared (the stored window with the oracle's bits, every other element with its sentinel), and every input buffer must come back
unchanged.  A case that takes an MFMA kernel runs a second time under debug key 0: the VALU kernel on the same strided operands
must store the same bits."""
import contextlib

import numpy as np
import pytest
import torch

import linear_cases as lc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@contextlib.contextmanager
def debug_keys(keys):
    from eam_rl4co_amd import _lib

    lib = _lib.load()
    for k in keys:
        assert lib.eamrl_debug_set(k, 1) == 0
    try:
        yield
    finally:
        for k in keys:
            lib.eamrl_debug_set(k, 0)


def view(buf, c, op):
    """The operand's window of its flat device buffer: [rows, cols] with row stride ld (bias: [out_dim])."""
    r, n, ld, off = lc.window(c, op)
    v = buf[lc.PAD + off:lc.PAD + off + r * ld].view(r, ld)[:, :n]
    return v[0] if op == "bias" else v


def device_call(name):
    """Device buffers of a case and its ops call: (inputs {op: (host buffer, device buffer)}, ybuf, fn, args, kwargs, the further
    kwargs of ops.linear_variant).  W goes in as the whole [out_dim, ldw] tensor with w_cols= wherever the window is narrower."""
    from eam_rl4co_amd import ops

    c, opnd = lc.CASES[name], lc.operands(name)
    inputs = {}
    for op in ("x", "W", "resw", "bias"):
        if opnd[op] is not None:
            host = lc.input_buffer(name, op)
            inputs[op] = (host, torch.from_numpy(host).to(DEV))
    ybuf = torch.from_numpy(lc.output_buffer(name)).to(DEV)
    out = view(ybuf.view(torch.float32), c, "y")
    x = view(inputs["x"][1], c, "x")
    assert x.data_ptr() % 16 == (4 * c["x"][1]) % 16 and out.data_ptr() % 16 == (4 * c["y"][1]) % 16
    if lc.wt(c):
        Wt = view(inputs["W"][1], c, "W")
        assert Wt.is_contiguous()
        return inputs, ybuf, ops.matmul_right, (x, Wt), dict(out=out), dict(transposed=True)
    ldw, woff = c["W"]
    kw = dict(out=out, relu=c["relu"])
    if ldw == c["in_dim"]:
        W = view(inputs["W"][1], c, "W")
    else:                               # the column window [woff, woff + in_dim) of a [out_dim, ldw] tensor
        W = inputs["W"][1][lc.PAD:lc.PAD + c["out_dim"] * ldw].view(c["out_dim"], ldw)
        kw["w_cols"] = (woff, woff + c["in_dim"])
    if c["bias"]:
        kw["bias"] = view(inputs["bias"][1], c, "bias")
    if c["res"]:
        kw["residual"] = view(inputs["resw"][1], c, "resw")
    if c["bn"]:
        kw["bn"] = tuple(torch.tensor(a, device=DEV) for a in opnd["bn"]) + (lc.EPS,)
    return inputs, ybuf, ops.linear, (x, W), kw, {}


def run_and_check(name, extra_keys=()):
    from eam_rl4co_amd import ops

    c = lc.CASES[name]
    inputs, ybuf, fn, args, kw, vkw = device_call(name)
    with debug_keys(c["keys"] + tuple(extra_keys)):
        variant = ops.linear_variant(*args, **kw, **vkw)
        ret = fn(*args, **kw)
    torch.cuda.synchronize()
    assert ret is kw["out"]
    lc.check_case(ybuf.cpu().numpy(), c)
    for op, (host, dev) in inputs.items():
        assert np.array_equal(dev.cpu().numpy().view(np.int32), host.view(np.int32)), f"{name}: input buffer {op} was written"
    return variant


@pytest.mark.parametrize("name", lc.NAMES)
def test_every_variant_stores_the_oracles_bits_and_nothing_else(oracle, name):
    c = lc.CASES[name]
    assert run_and_check(name) == lc.VARIANTS[c["variant"]]
    if c["variant"] in lc.MFMA:
        assert run_and_check(name, extra_keys=(0,)) == lc.VARIANTS["VALU"]


def test_linear_copies_an_x_with_a_strided_inner_dimension(oracle):
    from eam_rl4co_amd import ops

    name = "mfma64_rt_out132"
    c, opnd = lc.CASES[name], lc.operands(name)
    wide = torch.full((c["rows"], 2 * c["in_dim"]), float("nan"), device=DEV)
    wide[:, ::2] = torch.tensor(opnd["x"], device=DEV)
    x = wide[:, ::2]
    assert x.stride(-1) == 2
    W, b = torch.tensor(opnd["W"], device=DEV), torch.tensor(opnd["bias"], device=DEV)
    y = ops.linear(x, W, b)
    assert np.array_equal(y.cpu().numpy().view(np.int32), lc.reference(name).view(np.int32))
    assert ops.linear_variant(x, W, b) == lc.VARIANTS["MFMA64_RT"]
    with pytest.raises(ValueError, match="bad x"):              # matmul_right makes no copy
        ops.matmul_right(x, W.t().contiguous())


def test_wrapper_rejects_what_the_kernels_cannot_take(oracle):
    from eam_rl4co_amd import ops

    x = torch.zeros(5, 8, device=DEV)
    W = torch.zeros(12, 16, device=DEV)
    with pytest.raises(TypeError, match="unit inner stride"):
        ops.linear(x, W[:, ::2])
    with pytest.raises(TypeError, match="unit inner stride"):
        ops.linear_variant(x, W[:, ::2])
    with pytest.raises(ValueError, match="in_dim mismatch"):
        ops.linear(x, W)
    with pytest.raises(ValueError, match="in_dim mismatch"):
        ops.linear(x, W, w_cols=(0, 4))
    W = W[:, :8]
    for bad in (torch.zeros(4, 12, device=DEV), torch.zeros(5, 11, device=DEV), torch.zeros(5, 24, device=DEV)[:, ::2]):
        with pytest.raises(ValueError, match="bad output buffer"):
            ops.linear(x, W, out=bad)
        with pytest.raises(ValueError, match="bad output buffer"):
            ops.linear_variant(x, W, out=bad)
    with pytest.raises(ValueError, match="bad residual"):
        ops.linear(x, W, residual=torch.zeros(5, 13, device=DEV))
    with pytest.raises(ValueError, match="not combined"):
        ops.linear(x, W, relu=True, bn=tuple(torch.ones(12, device=DEV) for _ in range(4)) + (1e-5,))
    Wt = torch.zeros(8, 12, device=DEV)
    with pytest.raises(ValueError, match="must be contiguous"):
        ops.matmul_right(x, torch.zeros(8, 24, device=DEV)[:, ::2])
    for bad in (torch.zeros(4, 12, device=DEV), torch.zeros(5, 13, device=DEV)):
        with pytest.raises(ValueError, match="bad output buffer"):
            ops.matmul_right(x, Wt, out=bad)
    with pytest.raises(ValueError, match="in_dim mismatch"):
        ops.matmul_right(x, torch.zeros(9, 12, device=DEV))
