"""Host: EAS-Lay without a GPU.  The float64 restatement (tests/eas_layer_ref.py) against the reference's own pointer with the layer
in place (tests/golden/eas_lay_pointer.npz, recorded by make_golden_eas_lay.py: logits to 1e-6 of the largest logit -- the tolerance
float32 reference outputs carry elsewhere in this suite --, gradients to 1e-5 of their largest entry); the new ABI entries
(declared, bound, refusing before any launch with their condition named); the pack / unpack pair; the reference's
initialisation; the order of the loss coefficients; the constructions that stay unsupported; and the ReLU guard of every case
of tests/eas_layer_cases.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import eas_layer_cases as ec
import eas_layer_ref as er
import reeval_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = er.E


def test_restatement_reproduces_the_references_pointer_with_the_layer():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "eas_lay_pointer.npz"))
    t = {k: torch.from_numpy(fx[k]) for k in fx.files}
    N, Q, _ = t["query"].shape
    assert (N, Q, t["key"].shape[1], t["key"].shape[2]) == (3, 6, 20, 128) and float(t["W2"].abs().max()) > 0 and float(t["b2"].abs().max()) > 0
    d = lambda x: x.double()
    heads, _, _ = rr.glimpse_logits(d(t["query"]), d(t["key"]), d(t["value"]), d(t["logit_key"]), t["mask"])
    lay = {k: d(t[k]).reshape(N, -1, E).squeeze(1).clone().requires_grad_() for k in er.PARAMS}
    logits = er.pointer_logits(heads, lay, d(t["Wout"]), d(t["logit_key"]))
    err = float((logits.detach() - d(t["logits"])).abs().max())
    top = float(t["logits"].abs().max())
    print(f"logits: max err {err:.3e}, max |logit| {top:.3e}")
    assert err <= 1e-6 * top
    grads = torch.autograd.grad((d(t["C"]) * logits).sum(), [lay[k] for k in er.PARAMS])
    for k, g in zip(er.PARAMS, grads):
        want = d(t["d" + k]).reshape(g.shape)
        e, top = float((g - want).abs().max()), float(want.abs().max())
        print(f"d{k}: max err {e:.3e}, max |entry| {top:.3e}")
        assert top > 0 and e <= 1e-5 * top


def test_new_entries_are_declared_and_bound():
    from eam_rl4co_amd import _lib, ops

    with open(os.path.join(ROOT, "include", "eamrl.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+eamrl_eas_layer\s*\{", text)
    assert re.search(r"\bint\s+eamrl_eas_layer_backward\s*\(\s*const\s+eamrl_reeval\s*\*\s*p\s*,\s*const\s+eamrl_eas_layer\s*\*\s*layer\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"\bint\s+eamrl_am_rollout_eas_layer\s*\(", text) and re.search(r"\bint\s+eamrl_rollout_eas_layer_supported\s*\(", text)
    for name in ("eamrl_eas_layer_backward", "eamrl_am_rollout_eas_layer", "eamrl_rollout_eas_layer_supported"):
        assert name in _lib.PROTOTYPES
    assert callable(ops.ReevalPlan.backward_layer) and callable(ops.rollout_eas_layer_supported)


def test_null_arguments_and_refusals_name_their_entry_and_condition():
    from eam_rl4co_amd import _lib

    lib = _lib.load()
    assert lib.eamrl_eas_layer_backward(None, None, None) == -1 and b"eamrl_eas_layer_backward" in lib.eamrl_last_error()
    assert lib.eamrl_am_rollout_eas_layer(_lib.ENV_TSP, None, None, None, 8, 0, None, None, 0, 0, 0, None, 10.0, 1.0, 20, None, None,
                                          None, None, None) == -1
    assert b"eamrl_am_rollout_eas_layer" in lib.eamrl_last_error()
    assert lib.eamrl_rollout_eas_layer_supported(_lib.ENV_TSP, None, 8) == 0
    s, ly = _lib.Reeval(), _lib.EasLayer()
    s.M = 113
    assert lib.eamrl_eas_layer_backward(C.byref(s), C.byref(ly), None) == -1
    assert b"eamrl_eas_layer_backward" in lib.eamrl_last_error() and b"p->M <= 112" in lib.eamrl_last_error()
    s.M, s.dyn = 20, 1 << 12
    assert lib.eamrl_eas_layer_backward(C.byref(s), C.byref(ly), None) == -1 and b"p->dyn == nullptr" in lib.eamrl_last_error()
    s.dyn = None
    assert lib.eamrl_eas_layer_backward(C.byref(s), C.byref(ly), None) == -1 and b"p->heads != nullptr" in lib.eamrl_last_error()


def test_supported_answers_on_the_host():
    from eam_rl4co_amd import _lib

    lib = _lib.load()

    def cache(M=20, B=2, E=128, H=8):
        c = _lib.Cache()
        c.ld, c.B, c.M, c.E, c.H = 6 * E, B, M, E, H
        return c

    sup = lambda env, c, R: lib.eamrl_rollout_eas_layer_supported(env, C.byref(c), R)
    assert sup(_lib.ENV_TSP, cache(), 4) == 1 and sup(_lib.ENV_CVRP, cache(21), 2 * 128) == 1 and sup(_lib.ENV_TSP, cache(112), 42) == 1
    assert sup(_lib.ENV_TSP, cache(113), 8) == 0 and sup(_lib.ENV_TSP, cache(), 2) == 0 and sup(_lib.ENV_TSP, cache(), 2 * 129) == 0
    assert sup(_lib.ENV_TSP, cache(E=64), 8) == 0 and sup(_lib.ENV_TSP, cache(H=4), 8) == 0 and sup(_lib.ENV_TSP, cache(), 7) == 0
    for env in (_lib.ENV_SDVRP, _lib.ENV_PCTSP, _lib.ENV_OP, _lib.ENV_CVRPTW, _lib.ENV_PDP):
        assert sup(env, cache(21), 8) == 0


def test_pack_unpack_round_trip_and_documented_order():
    from eam_rl4co_amd import ops

    W = torch.randn(3, E, E, generator=torch.Generator().manual_seed(5))
    P = ops.pack_eas_layer(W)
    assert P.shape == (3, E * E) and torch.equal(ops.unpack_eas_layer(P), W) and torch.equal(ops.pack_eas_layer(ops.unpack_eas_layer(P)), P)
    for b in range(3):      # the fragment order of the transpose, instance by instance
        assert torch.equal(P[b], ops.pack_mfma_a(W[b].t().contiguous()))
    for T, q, l, i in ((0, 0, 0, 0), (3, 5, 17, 2), (7, 7, 63, 3)):       # the header's formula
        assert P[1, 4 * ((T * 8 + q) * 64 + l) + i] == W[1, 16 * q + 4 * i + l // 16, 16 * T + l % 16]


def test_initialisation_is_the_references():
    from eam_rl4co_amd.search import eas_layer_init

    N = 16
    W1, b1, W2, b2 = eas_layer_init(N, E, torch.Generator().manual_seed(3))
    assert W1.shape == (N, E, E) and b1.shape == (N, 1, E) and W2.shape == (N, E, E) and b2.shape == (N, 1, E)
    bw, bb = math.sqrt(6 / (E * E + N * E)), math.sqrt(6 / (E + N * E))
    assert float(W1.abs().max()) <= bw and float(W1.abs().max()) > bw / 2
    assert float(b1.abs().max()) <= bb and float(b1.abs().max()) > bb / 2
    assert not W2.any() and not b2.any()
    again = eas_layer_init(N, E, torch.Generator().manual_seed(3))
    assert torch.equal(again[0], W1) and torch.equal(again[1], b1)


def test_coefficient_rows_are_in_s_b_order_with_the_forced_row_last():
    from eam_rl4co_amd.search import eas_layer_row_coefficients, eas_loss_coefficients

    B, A, S = 2, 3, 4
    reward = torch.randn(B, A, S, generator=torch.Generator().manual_seed(1))
    coef = eas_loss_coefficients(reward, "multistart", 0.013, incumbent=True)
    rows = eas_layer_row_coefficients(coef)
    assert rows.shape == ((S + 1) * A * B,)
    for g in range(S + 1):
        for a in range(A):
            for b in range(B):
                assert rows[(g * A + a) * B + b] == coef[b, a, g]
    assert torch.equal(rows[S * A * B:], torch.full((A * B,), -0.013 / (B * A)))
    assert eas_layer_row_coefficients(eas_loss_coefficients(reward, "multistart", 0.013, incumbent=False)).shape == (S * A * B,)


def test_a_layer_search_off_the_gpu_raises_before_anything_else():
    import eam_rl4co_amd as ea

    env = ea.get_env("tsp", generator_params=dict(num_loc=10))
    pol = ea.AttentionModelPolicy(env_name="tsp").eval()
    for make in (lambda: ea.EASLay(env, pol), lambda: ea.EAS(env, pol, use_eas_layer=True),     # (the second: both flags)
                 lambda: ea.EAS(env, pol, use_eas_layer=True, use_eas_embedding=False, num_parallel_runs=2)):
        with pytest.raises(NotImplementedError, match="no CPU path"):
            make()
    assert "no CPU path" in ea.EAS.__doc__


@pytest.mark.parametrize("name", ec.NAMES)
def test_every_case_meets_its_relu_guard(name):
    c = ec.CASES[name]
    assert c["M"] <= 112 and not c["dyn"] and name in ec.SEEDS
    op, glogp, lay, heads, r64, r32 = ec.reference(name)
    assert float(lay["W2"].abs().max()) > 0 and heads.shape == (c["B"] * c["S"], c["T"], E)
    lo, err = ec.guard_figures(op, lay, heads)
    print(f"{name}: min |pre64| {lo:.3e}, max |pre32 - pre64| {err:.3e}, ratio {lo / err:.1f}")
    assert lo >= ec.GUARD * err
    live = r64["active"]
    assert bool(((r64["pre"] > 0) == (r32["pre"] > 0))[live].all())
    assert 0.05 < float((r64["pre"] > 0)[live].float().mean()) < 0.95          # both sides of the kink are populated
    for g in er.GRADS:
        assert float(r64[g].abs().max()) > 0 and ec.bound(name, g, r64, r32) > 0


def test_the_cases_cover_the_shapes_the_kernels_branch_on():
    cs = list(ec.CASES.values())
    assert {c["M"] for c in cs} >= {20, 33, 64, 65, 112} and {c["S"] for c in cs} >= {2, 16, 17, 128} and {c["B"] for c in cs} >= {1, 3, 100}
    assert {c["tstart"] for c in cs} == {0, 1} and {c["clip"] for c in cs} == {0.0, 10.0} and {c["temp"] for c in cs} == {1.0, 0.7}
    assert {c["lse"] for c in cs} == {True, False} and any(c["forced"] for c in cs)
    assert any(c["B"] == 100 and c["nchunk"] == 1 for c in cs)
