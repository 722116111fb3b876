"""GPU: the Heterogeneous Attention Model (HAM) for pickup and delivery.

Kernels (ops.hetero_mha, ops.hetero_mha_backward; csrc/hetero_attn.hip) against the float64 run of tests/ham_ref.py on the cases
and under the bounds of tests/ham_cases.py; the policy against rollouts, embeddings and gradients recorded from the reference
(tests/golden/make_golden_ham.py).  Every figure is printed before it is asserted.

Measured on the MI355X, kernel error over the error of the restatement's float32 run (bound: MARGIN = 4), the largest over the
cases and where: forward y 1.45 at M513_B2 (1.19 at M17_B3 among the small ones, 0.45 .. 1.10 elsewhere); backward dproj 1.72 at
M3_B1, 1.15 .. 1.41 from M = 5 to 129; the peaked cases are exact in the forward (both runs give the one-hot row) and 1.00 in the
backward, the all-equal cases 0.88 .. 1.01; the cases with the pair or the same-role scores 100 above the general ones 0.80 .. 1.72
(y, 1.0e-8 against 6.0e-9 at M101_B2_pair_high) and 1.00 .. 1.02 (dproj).  The depot row was bit-equal to ops.mha_encoder.  Rollouts: tours identical on all six
fixtures, summed log-likelihood at most 3.1e-5 away (one float32 ulp at |ll| ~ 500, PDP-100).  Embeddings 1.43e-6 (batch norm) and
1.97e-6 (instance norm) from the reference's.  The REINFORCE step's largest relative gradient-norm difference: 1.4e-6.
"""
import os

import numpy as np
import pytest
import torch

import ham_cases as hc
import ham_ref
from _util import golden

pytestmark = pytest.mark.gpu

DEV = "cuda"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_policy(cfg="am", **kw):
    import eam_rl4co_amd as ea

    if cfg == "pomo":
        kw = dict(hc.POMO, **kw)
    pol = ea.HeterogeneousAttentionModelPolicy(**kw).eval()
    sd = pol.state_dict()
    for k, v in hc.weights(cfg).items():
        sd[k].copy_(torch.from_numpy(v))
    return pol.to(DEV)


def make_td(locs):
    """Post-reset TensorDict on the GPU from recorded locs [B, N + 1, 2] (depot first)."""
    import eam_rl4co_amd as ea

    env = ea.PDPEnv(generator_params=dict(num_loc=locs.shape[1] - 1))
    td = ea.TensorDict({"locs": torch.from_numpy(np.ascontiguousarray(locs[:, 1:])),
                        "depot": torch.from_numpy(np.ascontiguousarray(locs[:, 0]))}, batch_size=[locs.shape[0]])
    return env, env.reset(td).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
def _report(name, out, got, r64, r32):
    c = hc.CASES[name]
    fig, f32, bd = hc.error(out, got, r64), hc.error(out, r32[out], r64), hc.bound(c, out, r64, r32)
    print(f"HAMK {name} {out} kernel {fig:.3e} float32-restatement {f32:.3e} ratio {fig / f32 if f32 else float('nan'):.2f} "
          f"bound {bd:.3e} floor {hc.U * r64['_scale'][out]:.3e} |ref| {r64['_scale'][out]:.3e}")
    return fig, bd


@pytest.mark.parametrize("name", hc.NAMES)
def test_forward_kernel_matches_the_float64_restatement(name):
    from eam_rl4co_amd import ops

    c = hc.CASES[name]
    op, r64, r32 = hc.reference(name)
    assert ops.hetero_mha_supported(c["M"], hc.E, hc.H)
    proj = op["proj"].to(DEV)
    a, b = ops.hetero_mha(proj, hc.H), ops.hetero_mha(proj, hc.H)
    torch.cuda.synchronize()
    fig, bd = _report(name, "y", a.cpu(), r64, r32)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)                            # no atomics: two runs are bit-equal
    assert fig <= bd
    if c["B"] > 1:                                      # an instance's result does not depend on the batch
        assert torch.equal(ops.hetero_mha(proj[-1:].contiguous(), hc.H)[0], a[-1])


@pytest.mark.parametrize("name", hc.BWD_NAMES)
def test_backward_kernel_matches_the_float64_restatement(name):
    from eam_rl4co_amd import ops

    c = hc.CASES[name]
    op, r64, r32 = hc.reference(name)
    assert ops.hetero_mha_backward_supported(c["M"], hc.E, hc.H)
    proj, dout = op["proj"].to(DEV), op["dout"].to(DEV)
    a, b = ops.hetero_mha_backward(proj, dout, hc.H), ops.hetero_mha_backward(proj, dout, hc.H)
    torch.cuda.synchronize()
    fig, bd = _report(name, "dproj", a.cpu(), r64, r32)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)                            # dk and dv are summed in a fixed order
    assert (a[:, 0, 3 * hc.E:] == 0).all()              # the depot's dqpair | dqsame | dqother are written as zeros
    assert fig <= bd


def test_depot_row_is_plain_attention():
    """The depot row has the M general scores only: it agrees with ops.mha_encoder on the q | k | v third within the case's bound."""
    from eam_rl4co_amd import ops

    for name in ("M33_B3", "M129_B3"):
        op, r64, r32 = hc.reference(name)
        proj = op["proj"].to(DEV)
        het = ops.hetero_mha(proj, hc.H)[:, 0]
        plain = ops.mha_encoder(proj[..., :3 * hc.E].contiguous(), hc.H)[:, 0]
        bd = hc.bound(hc.CASES[name], "y", r64, r32)
        fig = float((het.double() - plain.double()).abs().max())
        print(f"HAMK {name} depot row: hetero against mha_encoder {fig:.3e} bound {bd:.3e}")
        assert fig <= bd
        assert float((plain.cpu().double() - r64["y"][:, 0]).abs().max()) <= bd


def test_depot_padding_is_never_read():
    """The depot's last 3E of proj are ignored: NaNs there change nothing."""
    from eam_rl4co_amd import ops

    op, _, _ = hc.reference("M21_B3")
    proj = op["proj"].to(DEV)
    bad = proj.clone()
    bad[:, 0, 3 * hc.E:] = float("nan")
    assert torch.equal(ops.hetero_mha(bad, hc.H), ops.hetero_mha(proj, hc.H))
    dout = op["dout"].to(DEV)
    assert torch.equal(ops.hetero_mha_backward(bad, dout, hc.H), ops.hetero_mha_backward(proj, dout, hc.H))


def test_unsupported_shapes_fail_with_the_requirement_message():
    from eam_rl4co_amd import ops

    assert not ops.hetero_mha_supported(hc.MAX_NODES + 2, hc.E, hc.H) and not ops.hetero_mha_supported(20, hc.E, hc.H)
    assert not ops.hetero_mha_backward_supported(hc.BWD_MAX_NODES + 2, hc.E, hc.H)
    with pytest.raises(RuntimeError, match="eamrl_hetero_mha: requirement failed"):
        ops.hetero_mha(torch.zeros(1, hc.MAX_NODES + 2, 6 * hc.E, device=DEV), hc.H)
    with pytest.raises(RuntimeError, match="eamrl_hetero_mha_backward: requirement failed"):
        ops.hetero_mha_backward(torch.zeros(1, 131, 6 * hc.E, device=DEV), torch.zeros(1, 131, hc.E, device=DEV), hc.H)
    with pytest.raises(AssertionError, match="Graph size should have odd number of nodes"):
        ops.hetero_mha(torch.zeros(1, 20, 6 * hc.E, device=DEV), hc.H)
    with pytest.raises(AssertionError, match="Graph size should have odd number of nodes"):
        ops.hetero_mha_backward(torch.zeros(1, 20, 6 * hc.E, device=DEV), torch.zeros(1, 20, hc.E, device=DEV), hc.H)
    with pytest.raises(ValueError, match="hetero_mha_backward: proj must be"):
        ops.hetero_mha_backward(torch.zeros(1, 21, 6 * hc.E + 1, device=DEV), torch.zeros(1, 21, hc.E, device=DEV), hc.H)


def test_module_forward_on_the_recorded_fixture():
    """HeterogenousMHA.forward (projections, kernel, W_out) against the reference module's float64 output."""
    from eam_rl4co_amd.policy import HeterogenousMHA

    for name in hc.MHA_FIXTURES:
        fx = golden(name)
        mod = HeterogenousMHA(8, 128, 128)
        with torch.no_grad():
            for k in ham_ref.WEIGHT_KEYS:
                getattr(mod, k).copy_(torch.from_numpy(fx[k]))
        mod = mod.to(DEV)
        with torch.no_grad():
            got = mod(t(fx["x"])).cpu().double()
        want = torch.from_numpy(fx["out"])
        f32 = float((torch.from_numpy(fx["out_float32"]).double() - want).abs().max())
        fig = float((got - want).abs().max())
        bd = hc.MARGIN * max(f32, hc.U * float(want.abs().max()))
        print(f"HAMK {name} module kernel {fig:.3e} reference-float32 {f32:.3e} bound {bd:.3e}")
        assert fig <= bd


# ---------------------------------------------------------------------------------------------------------------------
# policy
# ---------------------------------------------------------------------------------------------------------------------
def call_kwargs(fx):
    kw = dict(return_sum_log_likelihood=False, decode_type=str(fx["decode_type"]))
    if int(fx["num_starts"]) > 1:
        kw["num_starts"] = int(fx["num_starts"])
    if "noise" in fx:
        kw["noise"] = t(fx["noise"])
    return kw


@pytest.mark.parametrize("name", hc.ROLLOUT_FIXTURES)
def test_policy_rollout_matches_the_reference(name):
    import pdp_ref

    fx = golden(name)
    assert float(fx["min_top2_gap"]) >= 1e-4
    pol = make_policy(hc.cfg_for(fx))
    env, td = make_td(fx["locs"])
    out = pol(td, env, phase="test", **call_kwargs(fx))
    acts = out["actions"].cpu().numpy()
    assert np.array_equal(acts, fx["actions"]), "tours"
    np.testing.assert_allclose(out["reward"].cpu().numpy(), fx["reward"], rtol=1e-6)
    ll = out["log_likelihood"].sum(1).cpu().numpy()
    print(f"HAMP {name} summed log-likelihood: max abs difference {np.abs(ll - fx['log_likelihood']).max():.3e}")
    np.testing.assert_allclose(ll, fx["log_likelihood"], rtol=2e-5, atol=2e-5)
    assert (pdp_ref.check_solution(acts, fx["locs"].shape[1] - 1) == pdp_ref.VALID).all()
    summed = pol(td, env, phase="test", **dict(call_kwargs(fx), return_sum_log_likelihood=True))
    np.testing.assert_allclose(summed["log_likelihood"].cpu().numpy(), fx["log_likelihood"], rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("tag,cfg", [("batch", "am"), ("instance", "pomo")])
def test_encoder_embeddings_match_the_reference(tag, cfg):
    fx = golden("ham_embed_pdp20")
    pol = make_policy(cfg)
    _, td = make_td(fx["locs"])
    with torch.no_grad():
        h, init = pol.encoder(td)
    fig = float((h.cpu().double() - torch.from_numpy(fx["embeddings_" + tag]).double()).abs().max())
    bd = hc.MARGIN * hc.EMBED_F32_DISTANCE[tag]
    print(f"HAMP embeddings {tag}: {fig:.3e} bound {bd:.3e}")
    assert float((init.cpu().double() - torch.from_numpy(fx["init_embeds_" + tag]).double()).abs().max()) <= 5e-7
    assert fig <= bd


def test_graphed_rollout_equals_eager():
    import eam_rl4co_amd as ea

    pol = make_policy()
    env = ea.get_env("pdp", generator_params=dict(num_loc=20), seed=3)
    tds = [env.reset(batch_size=[16]).to(DEV) for _ in range(2)]
    g = ea.GraphedRollout(pol, env, tds[0], decode_type="greedy")

    def same(td):
        a = g(td)
        b = pol(td.clone(), env, phase="test", decode_type="greedy")
        for k in ("actions", "reward", "log_likelihood"):
            assert torch.equal(a[k], b[k]), k

    for td in tds + [tds[0]]:
        same(td)
    with torch.no_grad():                               # a changed parameter is repacked into the buffers the graph reads
        pol.encoder.layers[1][0].module.W2_query.mul_(1.5)
    same(tds[1])


def test_bf16_mixed_keeps_raising():
    with pytest.raises(NotImplementedError, match="GraphAttentionNetwork"):
        make_policy(precision="bf16-mixed")


# ---------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------
def _attention_paths(name):
    """(native, torch) results {"y", "dproj"} of train._hetero_attention on the operands of case `name`."""
    from eam_rl4co_amd import train

    op, _, _ = hc.reference(name)
    res = []
    for env in ("0", "1"):
        old = os.environ.get("EAMRL_TORCH_ATTENTION")
        os.environ["EAMRL_TORCH_ATTENTION"] = env
        try:
            p = op["proj"].to(DEV).requires_grad_(True)
            y = train._hetero_attention(p, hc.H)
            assert (type(y.grad_fn).__name__ == "_HeteroAttentionFnBackward") == (env == "0")
            (d,) = torch.autograd.grad(y, p, op["dout"].to(DEV))
        finally:
            if old is None:
                del os.environ["EAMRL_TORCH_ATTENTION"]
            else:
                os.environ["EAMRL_TORCH_ATTENTION"] = old
        res.append(dict(y=y.detach().cpu(), dproj=d.cpu()))
    return res


@pytest.mark.parametrize("name", ["M21_B3", "M101_B3"])
def test_native_backward_equals_the_torch_expression(name):
    """The native forward + backward and the EAMRL_TORCH_ATTENTION=1 cross-check path: each within the kernel bound of the float64
    restatement, and within the same bound of each other.  Measured: y 1.9e-6 (bound 5.1e-6) and dproj 3.2e-5 (9.0e-5) at
    M21_B3, y 2.9e-6 (1.0e-5) and dproj 7.6e-5 (2.5e-4) at M101_B3."""
    c = hc.CASES[name]
    _, r64, r32 = hc.reference(name)
    native, torch_path = _attention_paths(name)
    for out in ("y", "dproj"):
        bd = hc.bound(c, out, r64, r32)
        figs = hc.error(out, native[out], r64), hc.error(out, torch_path[out], r64)
        d = native[out].double() - torch_path[out].double()
        mutual = float(d.abs().max()) if out == "y" else float(d.norm())
        print(f"HAMT {name} {out} native {figs[0]:.3e} torch {figs[1]:.3e} mutual {mutual:.3e} bound {bd:.3e}")
        assert figs[0] <= bd and figs[1] <= bd and mutual <= bd


def test_graph_encoder_is_not_claimed_bit_equal():
    from eam_rl4co_amd import train

    fx = golden("ham_pdp20_greedy")
    _, td = make_td(fx["locs"])
    assert train.graph_encoder_equals_native(make_policy("pomo"), td) is False


def test_reinforce_step_matches_the_reference_gradients():
    """REINFORCE.shared_step with the "no" baseline (reinforce.py:59-106) on the policy in train() mode, against the step recorded
    from the reference: tours, reward, log-likelihood, loss, running statistics and every parameter's gradient, held to the
    criterion of tests/test_gpu_train.py (1e-4 of the norm)."""
    fx = golden("train_ham_pdp20")
    pol = make_policy().train()
    env, td = make_td(fx["locs"])
    out = pol(td, env, phase="train", select_best=False, decode_type="sampling", noise=t(fx["noise"]))
    assert np.array_equal(out["actions"].cpu().numpy(), fx["actions"]), "actions"
    np.testing.assert_allclose(out["reward"].cpu().numpy(), fx["reward"], rtol=1e-6)
    ll = out["log_likelihood"]
    assert ll.requires_grad and ll.grad_fn is not None
    np.testing.assert_allclose(ll.detach().cpu().numpy(), fx["logp_steps"].sum(1), rtol=2e-5, atol=2e-5)
    for k in fx:
        if k.startswith("buf__"):
            np.testing.assert_allclose(dict(pol.named_buffers())[k[5:]].cpu().numpy(), fx[k], rtol=0, atol=1e-6)
    loss = -(out["reward"] * ll).mean()
    np.testing.assert_allclose(float(loss.detach()), float(fx["loss"]), rtol=2e-5)
    loss.backward()
    params = dict(pol.named_parameters())
    total_ref = float(np.sqrt((fx["grad_norms"] ** 2).sum()))
    worst = 0.0
    for k, ref_norm in zip(fx["grad_names"], fx["grad_norms"]):
        g = params[str(k)].grad
        got = 0.0 if g is None else float(g.double().norm())
        worst = max(worst, abs(got - ref_norm) / max(ref_norm, 1e-3 * total_ref))
    print(f"HAMT train_ham_pdp20: largest relative gradient-norm difference {worst:.3e}")
    for k, ref_norm in zip(fx["grad_names"], fx["grad_norms"]):
        g = params[str(k)].grad
        got = 0.0 if g is None else float(g.double().norm())
        assert abs(got - ref_norm) <= 1e-4 * max(ref_norm, 1e-3 * total_ref) + 1e-7, (str(k), got, ref_norm)
        if "grad__" + str(k) in fx and g is not None:
            ref = fx["grad__" + str(k)]
            np.testing.assert_allclose(g.cpu().numpy(), ref, rtol=0, atol=1e-4 * max(float(np.abs(ref).max()), 1e-3 * total_ref),
                                       err_msg=str(k))
