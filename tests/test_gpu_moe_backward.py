"""GPU: the native sparse forward and backward of the MoE sublayer's experts (eamrl_moe_experts_forward / _backward,
train._MoEExpertsFn).  The forward against ops.moe_ffn BIT FOR BIT on its own routing; every gradient against the float64
statement tests/moe_grad_ref.py with the routing passed explicitly (no near-tie can flip a selection), bounded by what the
fp32 torch expression (`moe_autograd`'s expert part: every expert on all rows, zero gates for the unselected) achieves on the
same device:

    err(T) = max |T - ref| / max |ref|,     err_native(T) <= 4 * err_torch(T) + 1e-7     for every output tensor T

(the margin tests/test_gpu_ptrnet.py grants a kernel whose summation order differs from torch's).  Every ratio is printed.

Measured on an MI355X, native error / torch error per output, the largest over all cases of this file: y 1.00, dx 1.17, dg 1.30,
dW1 1.11, db1 1.24, dW2 1.18, db2 1.85 (both errors between 1e-7 and 7e-7); DESIGN.md section 16 "Native backward" has them
with the timings of tools/time_moe_train.py.
"""
import numpy as np
import pytest
import torch

import moe_grad_ref
import moe_ref
from _util import golden
from test_gpu_moe import SHAPES, make_policy, pack, sublayer_case
from test_gpu_parity import DEV, make_td, t

pytestmark = pytest.mark.gpu

OUTS = ("y", "dx", "dg", "dW1", "db1", "dW2", "db2")
GRAD_ROWS = (1, 15, 16, 17, 63, 64, 65, 129, 257)          # the 16- and 64-row boundaries, more than one 64-row group
GRAD_SHAPES = ((4, 2), (8, 2), (4, 4), (2, 1), (1, 1))
WORST = {}


def packs_of(c):
    from eam_rl4co_amd import ops

    W1, b1, W2, b2 = ([t(c[nm][e]) for e in range(c["W1"].shape[0])] for nm in ("W1", "b1", "W2", "b2"))
    return dict(ops.pack_moe_experts(W1, b1, W2, b2), **ops.pack_moe_experts_backward(W1, W2))


def native(c, pk=None, **need):
    """One forward and backward through the ops wrappers -> dict of the outputs (device tensors) and the state."""
    from eam_rl4co_amd import ops

    pk = packs_of(c) if pk is None else pk
    x, sel, g, dy = t(c["x"]), t(c["sel"]), t(c["g"]), t(c["dy"])
    y, state = ops.moe_experts_forward(x, sel, g, pk)
    dx, dg, dW1, db1, dW2, db2 = ops.moe_experts_backward(dy, x, g, pk, state, **need)
    return dict(y=y, dx=dx, dg=dg, dW1=dW1, db1=db1, dW2=dW2, db2=db2, state=state)


def torch_expression(c):
    """The expert part of train.moe_autograd in fp32 on the device, on the given routing."""
    from eam_rl4co_amd import train

    n = c["W1"].shape[0]
    x, g = t(c["x"]).requires_grad_(True), t(c["g"]).requires_grad_(True)
    par = {nm: [t(c[nm][e]).requires_grad_(True) for e in range(n)] for nm in ("W1", "b1", "W2", "b2")}
    sel = t(c["sel"]).long()
    ok = (sel >= 0) & (sel < n)
    gates = torch.zeros(x.shape[0], n + 1, device=DEV).scatter(-1, torch.where(ok, sel, torch.full_like(sel, n)), g)[:, :n]
    y = None
    for e in range(n):
        o = train._linear(train._linear(x, par["W1"][e], par["b1"][e], relu=True), par["W2"][e], par["b2"][e])
        o = gates[:, e:e + 1] * o
        y = o if y is None else y + o
    y.backward(t(c["dy"]))
    out = dict(y=y.detach(), dx=x.grad, dg=g.grad)
    for key, nm in (("dW1", "W1"), ("db1", "b1"), ("dW2", "W2"), ("db2", "b2")):
        out[key] = torch.stack([p.grad for p in par[nm]])
    return out


def check_against_float64(c, what):
    ref = moe_grad_ref.experts_grad_ref(**c)
    got, tor = native(c), torch_expression(c)
    for key in OUTS:
        scale = float(np.abs(ref[key]).max())
        assert scale > 0, (what, key)
        e_nat = float(np.abs(got[key].double().cpu().numpy() - ref[key]).max()) / scale
        e_tor = float(np.abs(tor[key].double().cpu().numpy() - ref[key]).max()) / scale
        ratio = e_nat / max(e_tor, 1e-12)
        WORST[key] = max(WORST.get(key, 0.0), ratio)
        print(f"MOEB {what} {key}: native {e_nat:.3e} torch {e_tor:.3e} ratio {ratio:.2f}")
        assert e_nat <= 4 * e_tor + 1e-7, (what, key, e_nat, e_tor)
    counts = np.bincount(c["sel"].reshape(-1).astype(np.int64), minlength=c["W1"].shape[0])
    for e in np.nonzero(counts == 0)[0]:          # an expert without rows: zero tensors, exactly
        for key in ("dW1", "db1", "dW2", "db2"):
            assert not got[key][e].any(), (what, key, int(e))
    return got, ref


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_exp,k", SHAPES)
def test_forward_is_bit_exact_on_the_routing_of_moe_ffn(n_exp, k):
    from eam_rl4co_amd import ops

    for gating in ("random", "skew"):
        for rows in (1, 17, 64, 65, 16 * 37 + 5):
            x, w_gate, experts, _ = sublayer_case(rows, n_exp, k, gating, 1000 * n_exp + 10 * k + rows)
            pk = pack(experts)
            want, sel, g = ops.moe_ffn(t(x), t(w_gate), pk, k, return_routing=True)
            y, state = ops.moe_experts_forward(t(x), sel, g, pk)
            assert torch.equal(y, want), f"n_exp={n_exp} k={k} rows={rows} {gating}"
            assert ops.moe_experts_dropped(state) == 0
            counts = state[:4 * n_exp].view(torch.int32).tolist()
            assert counts == torch.bincount(sel.reshape(-1).long(), minlength=n_exp).tolist()


def test_row_lists_are_in_ascending_row_order():
    """The deterministic-list rule: every expert's list holds its rows in ascending order (the weight gradients sum over it)."""
    from eam_rl4co_amd import ops

    c = moe_grad_ref.make_case(1000, 4, 2, 21)
    _, state = ops.moe_experts_forward(t(c["x"]), t(c["sel"]), t(c["g"]), packs_of(c))
    lists = state[64:64 + 16 * 1000].view(torch.int32).view(4, 1000).cpu().numpy()
    counts = state[:16].view(torch.int32).tolist()
    for e in range(4):
        rows_of_e, slots = np.nonzero(c["sel"] == e)
        assert counts[e] == len(rows_of_e)
        assert np.array_equal(lists[e, :counts[e]], rows_of_e * 8 + slots)


# ---------------------------------------------------------------------------------------------------------------------
# gradients against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_exp,k", GRAD_SHAPES)
def test_gradients_against_float64(n_exp, k):
    for rows in GRAD_ROWS:
        c = moe_grad_ref.make_case(rows, n_exp, k, 100 * n_exp + 10 * k + rows)
        check_against_float64(c, f"n_exp={n_exp} k={k} rows={rows}")
    print("MOEB largest native / torch error ratio so far:", {key: round(v, 2) for key, v in WORST.items()})


@pytest.mark.parametrize("name,rows,n_exp,k,routing", [("one expert without rows", 65, 4, 2, "skip_last"),
                                                       ("every row on expert 0", 129, 4, 2, "all_on_0"),
                                                       ("counts 1, 16, 17, 64", 98, 4, 1, (1, 16, 17, 64))])
def test_gradients_on_uneven_routings(name, rows, n_exp, k, routing):
    c = moe_grad_ref.make_case(rows, n_exp, k, 77, routing=routing)
    counts = np.bincount(c["sel"].reshape(-1).astype(np.int64), minlength=n_exp).tolist()
    if routing == "skip_last":
        assert counts[-1] == 0
    elif routing == "all_on_0":
        assert counts[0] == rows
    else:
        assert counts == list(routing)
    got, ref = check_against_float64(c, name)
    print("MOEB largest native / torch error ratio so far:", {key: round(v, 2) for key, v in WORST.items()})


def test_bad_selection_entries_are_dropped_on_the_device():
    """Entries outside 0 .. n_exp - 1 and repeats within a row contribute nothing, get dg = 0 and are counted; the rest of the
    batch is computed as if those slots were absent."""
    from eam_rl4co_amd import ops

    c = moe_grad_ref.make_case(70, 4, 2, 9)
    bad = c["sel"].copy()
    bad[3, 1], bad[17, 0], bad[40, 1], bad[69, 0] = 4, -1, bad[40, 0], 127
    clean = bad.copy()
    clean[3, 1] = clean[17, 0] = clean[40, 1] = clean[69, 0] = -1
    ref = moe_grad_ref.experts_grad_ref(**dict(c, sel=clean))
    got = native(dict(c, sel=bad))
    assert ops.moe_experts_dropped(got["state"]) == 4
    tor = torch_expression(dict(c, sel=clean))
    for key in OUTS:
        scale = float(np.abs(ref[key]).max())
        e_nat = float(np.abs(got[key].double().cpu().numpy() - ref[key]).max()) / scale
        e_tor = float(np.abs(tor[key].double().cpu().numpy() - ref[key]).max()) / scale
        print(f"MOEB dropped entries {key}: native {e_nat:.3e} torch {e_tor:.3e}")
        assert e_nat <= 4 * e_tor + 1e-7, key
    dg = got["dg"].cpu().numpy()
    assert dg[3, 1] == 0 and dg[17, 0] == 0 and dg[40, 1] == 0 and dg[69, 0] == 0


# ---------------------------------------------------------------------------------------------------------------------
# determinism, needs_input_grad
# ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    c = moe_grad_ref.make_case(257, 4, 2, 31)
    pk = packs_of(c)
    a, b = native(c, pk), native(c, pk)
    for key in OUTS:
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(a["state"][:64], b["state"][:64]), "counters"
    counts = a["state"][:16].view(torch.int32).tolist()
    la, lb = (s["state"][64:64 + 16 * 257].view(torch.int32).view(4, 257) for s in (a, b))
    for e in range(4):          # (a list's tail past its count is never written)
        assert torch.equal(la[e, :counts[e]], lb[e, :counts[e]]), f"row list of expert {e}"


def test_frozen_experts_produce_only_dx_and_dg(monkeypatch):
    from eam_rl4co_amd import ops, train

    c = moe_grad_ref.make_case(129, 4, 2, 41)
    pk = packs_of(c)
    asked = []
    orig = ops.moe_experts_backward

    def recording(*a, **kw):
        asked.append((kw["need_dx"], kw["need_dg"], kw["need_weight_grads"]))
        res = orig(*a, **kw)
        asked.append(tuple(r is not None for r in res))
        return res

    monkeypatch.setattr(ops, "moe_experts_backward", recording)
    outs = []
    for frozen in (False, True):
        x, g = t(c["x"]).requires_grad_(True), t(c["g"]).requires_grad_(True)
        params = [t(c[nm][e]).requires_grad_(not frozen) for nm in ("W1", "b1", "W2", "b2") for e in range(4)]
        y = train._MoEExpertsFn.apply(x, g, t(c["sel"]), pk, *params)
        y.backward(t(c["dy"]))
        outs.append((y.detach(), x.grad, g.grad, params))
    assert asked == [(True, True, True), (True,) * 6, (True, True, False), (True, True, False, False, False, False)]
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)
    assert all(p.grad is not None for p in outs[0][3]) and all(p.grad is None for p in outs[1][3])
    ref = moe_grad_ref.experts_grad_ref(**c)
    np.testing.assert_allclose(outs[0][3][0].grad.cpu().numpy(), ref["dW1"][0], rtol=0, atol=1e-5 * np.abs(ref["dW1"]).max())
    # packs=None: the function packs the parameters itself, the same bits
    x = t(c["x"]).requires_grad_(True)
    y = train._MoEExpertsFn.apply(x, t(c["g"]), t(c["sel"]).long(), None, *outs[1][3])
    assert torch.equal(y, outs[0][0])


# ---------------------------------------------------------------------------------------------------------------------
# the policy
# ---------------------------------------------------------------------------------------------------------------------
def test_reinforce_step_equals_the_torch_expression_path(monkeypatch):
    """One REINFORCE step with noisy gating on, the same torch seed: the native path against EAMRL_MOE_NATIVE_BACKWARD=0 --
    identical actions and routing, log-likelihood within 2e-5, every parameter's gradient within 1e-4 of the larger of its norm
    and 1e-3 of the total norm (the criterion of test_gpu_moe.py::test_reinforce_step_matches_the_reference_gradients)."""
    from eam_rl4co_amd import ops, train

    fx = golden("train_moe_cvrp20")
    env, td = make_td("cvrp", fx["locs"], fx["demand"])
    sort = torch.sort
    res = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("EAMRL_MOE_NATIVE_BACKWARD", switch)
        routing, native_calls = [], []

        def recording(*a, **kw):
            out = sort(*a, **kw)
            if kw.get("stable") and kw.get("descending"):
                routing.append(out[1][:, :2].clone())
            return out

        monkeypatch.setattr(torch, "sort", recording)
        fwd = ops.moe_experts_forward
        monkeypatch.setattr(ops, "moe_experts_forward", lambda *a: native_calls.append(1) or fwd(*a))
        pol = make_policy("am_cvrp_moe", fx).train()
        torch.manual_seed(7)
        # (sampling draws from torch's generator too: the fixture's recorded decoding noise covers only the steps of the tours
        # the reference sampled with noisy gating off)
        out = train.reinforce_loss(pol, env, td.clone(), baseline="no")
        out["loss"].backward()
        monkeypatch.setattr(torch, "sort", sort)
        monkeypatch.setattr(ops, "moe_experts_forward", fwd)
        assert len(native_calls) == (3 if switch == "1" else 0), "the switch chooses the path"
        res[switch] = (out, routing, {k: p.grad for k, p in pol.named_parameters()})
    (a, ra, ga), (b, rb, gb) = res["1"], res["0"]
    assert torch.equal(a["actions"], b["actions"]), "actions"
    assert len(ra) == len(rb) == 3 and all(torch.equal(p, q) for p, q in zip(ra, rb)), "routing"
    lla, llb = a["log_likelihood"].detach().cpu().numpy(), b["log_likelihood"].detach().cpu().numpy()
    print(f"MOEB policy: |ll native - ll torch| max {np.abs(lla - llb).max():.3e}")
    np.testing.assert_allclose(lla, llb, rtol=0, atol=2e-5)
    total = float(torch.sqrt(sum(g.double().pow(2).sum() for g in gb.values() if g is not None)))
    worst = 0.0
    for key, ref in gb.items():
        got = ga[key]
        assert (got is None) == (ref is None), key
        if ref is None:
            continue
        nr, ng = float(ref.double().norm()), float(got.double().norm())
        bound = 1e-4 * max(nr, 1e-3 * total)
        worst = max(worst, abs(ng - nr) / max(nr, 1e-3 * total))
        assert abs(ng - nr) <= bound + 1e-7, (key, ng, nr)
        assert float((got - ref).abs().max()) <= 1e-4 * max(float(ref.abs().max()), 1e-3 * total), key
    print(f"MOEB policy: largest relative gradient-norm difference {worst:.3e}")
    for li in range(3):
        for nm in ("w_gate", "w_noise"):
            assert float(ga[f"encoder.net.layers.{li}.2.module.{nm}"].abs().sum()) > 0, (li, nm)
