"""GPU: the MoE encoder (MVMoE).  The sublayer's three kernels (gate, grouped expert GEMM, combine) and whole rollouts of the
MoE policy against tests/moe_ref.py BIT FOR BIT -- both sides evaluate the same defined order -- and hence against the results
recorded from the reference (tests/test_host_moe.py pins moe_ref to those); one training step against the reference's
recorded gradients.  Every figure is printed before it is asserted.
"""
import os

import numpy as np
import pytest
import torch

import goldweights
import moe_ref
from _util import golden, golden_weights
from test_gpu_parity import DEV, assert_bits_equal, make_td, t

pytestmark = pytest.mark.gpu

POMO = dict(num_encoder_layers=6, normalization="instance", use_graph_context=False)
ROWS = (1, 15, 16, 17, 21, 49, 64, 65, 16 * 37 + 5)      # 16-row tiles, four of them per expert workgroup
SHAPES = ((4, 2), (4, 1), (4, 4), (2, 1), (8, 2))
f32 = np.float32


def make_policy(cfg, fx=None, moe_kwargs=None, **kw):
    import eam_rl4co_amd as ea

    if cfg.startswith("pomo"):
        kw = dict(POMO, **kw)
    pol = ea.AttentionModelPolicy(env_name=cfg.split("_")[1], moe_kwargs=moe_kwargs or moe_ref.MOE_KWARGS, **kw).eval()
    sd = pol.state_dict()
    for k, v in moe_ref.weights(cfg, fx).items():
        sd[k].copy_(torch.from_numpy(v))
    return pol.to(DEV)


def call_kwargs(fx):
    kw = dict(return_sum_log_likelihood=False)
    decode_type = str(fx["decode_type"])
    if decode_type == "evaluate":
        kw["actions"] = t(fx["actions"])
        decode_type = "sampling"
    kw["decode_type"] = decode_type
    if int(fx["num_starts"]) > 1:
        kw["num_starts"] = int(fx["num_starts"])
    if "noise" in fx:
        kw["noise"] = t(fx["noise"])
    return kw


# ---------------------------------------------------------------------------------------------------------------------
# the sublayer alone
# ---------------------------------------------------------------------------------------------------------------------
def sublayer_case(rows, n_exp, k, gating, seed):
    """Inputs of one sublayer call.  x[:, 0] = 1 is a bias feature, so w_gate[0] shifts an expert's logit for every row:
    gating "skew": expert 0 far above (every row selects it: with rows = 1, 17, 49 or 65 its list ends in a 1-row tile) and, where
    k < n_exp, the last expert far below (no row selects it: an empty list); "random": a free gate.  The last row is all
    zeros: its logits tie exactly."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, 128)).astype(f32)
    x[:, 0] = 1.0
    x[-1] = 0.0
    w_gate = (rng.standard_normal((128, n_exp)) / np.sqrt(128)).astype(f32)
    if gating == "skew":
        w_gate[0, 0] = 30.0
        if k < n_exp:
            w_gate[0, n_exp - 1] = -30.0
    experts = [((rng.uniform(-1, 1, (512, 128)) / np.sqrt(128)).astype(f32), rng.uniform(-0.1, 0.1, 512).astype(f32),
                (rng.uniform(-1, 1, (128, 512)) / np.sqrt(512)).astype(f32), rng.uniform(-0.1, 0.1, 128).astype(f32))
               for _ in range(n_exp)]
    bn = (rng.uniform(0.8, 1.2, 128).astype(f32), rng.uniform(-0.1, 0.1, 128).astype(f32), rng.uniform(-0.1, 0.1, 128).astype(f32),
          rng.uniform(0.5, 1.5, 128).astype(f32), 1e-5)
    return x, w_gate, experts, bn


def pack(experts):
    from eam_rl4co_amd import ops

    return ops.pack_moe_experts(*([t(ex[i]) for ex in experts] for i in range(4)))


@pytest.mark.parametrize("with_bn", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("n_exp,k", SHAPES)
def test_sublayer_bit_exact(n_exp, k, with_bn):
    from eam_rl4co_amd import ops

    for gating in ("random", "skew"):
        for rows in ROWS:
            x, w_gate, experts, bn = sublayer_case(rows, n_exp, k, gating, 1000 * n_exp + 10 * k + rows)
            want, p, sel_ref, g_ref = moe_ref.sublayer(x, w_gate, experts, k, bn=bn if with_bn else None)
            counts = np.bincount(sel_ref.reshape(-1).astype(np.int64), minlength=n_exp)
            if gating == "skew":
                if rows > 1:            # (the all-zero row ties and takes experts 0 .. k - 1)
                    assert counts[0] == rows, "one expert receives every row"
                if k < n_exp and rows > 1:
                    assert counts[n_exp - 1] == 0, "one expert receives no row"
                if rows in (1, 17, 49, 65):
                    assert counts[0] % 16 == 1, "a list ends in a 1-row tile"
            assert (sel_ref[-1] == np.arange(k)).all() and len(set(p[-1].tolist())) == 1, "the last row ties exactly"
            dx = t(x)
            dbn = tuple(t(v) for v in bn[:4]) + (bn[4],) if with_bn else None
            pk = pack(experts)
            outs = [ops.moe_ffn(dx, t(w_gate), pk, k, residual=dx, bn=dbn, return_routing=True) for _ in range(2)]
            what = f"n_exp={n_exp} k={k} rows={rows} {gating}"
            assert_bits_equal(outs[0][1], sel_ref, f"sel ({what})")
            assert_bits_equal(outs[0][2], g_ref, f"gates ({what})")
            assert_bits_equal(outs[0][0], want, f"output ({what})")
            for a, b in zip(outs[0], outs[1]):          # the row lists' order may differ between runs; no value may
                assert torch.equal(a, b), f"second run ({what})"


def test_sublayer_in_place_and_without_residual():
    from eam_rl4co_amd import ops

    x, w_gate, experts, bn = sublayer_case(53, 4, 2, "random", 7)
    y_ref, _, _, _ = moe_ref.moe(x, w_gate, experts, 2)
    pk = pack(experts)
    assert_bits_equal(ops.moe_ffn(t(x), t(w_gate), pk, 2), y_ref, "MoE(x) without a residual")
    h = t(x)
    out = ops.moe_ffn(h, t(w_gate), pk, 2, residual=h, out=h)
    assert out.data_ptr() == h.data_ptr()
    assert_bits_equal(out, moe_ref.sublayer(x, w_gate, experts, 2)[0], "in place")


def module_weights(fx):
    pre = str(fx["key_prefix"])
    sd = {}
    for key, shape in [("w_gate", (128, 4)), ("w_noise", (128, 4))] + [
            (f"experts.{e}.lins.{i}.{wb}", s) for e in range(4)
            for i, wb, s in ((0, "weight", (512, 128)), (0, "bias", (512,)), (1, "weight", (128, 512)), (1, "bias", (128,)))]:
        sd[pre + key] = goldweights.tensor_for(pre + key, shape)
    return pre, sd


def test_noisy_gating_on_the_recorded_draw():
    """The training-mode module with the reference's recorded standard-normal draw: the kernels against moe_ref bit for bit
    and against the reference's output; through the module (`MoE.sublayer(noise=)`), which is how a training-mode rollout runs."""
    from eam_rl4co_amd.policy import MoE

    fx = golden("moe_module_train")
    pre, sd = module_weights(fx)
    m = MoE(128, 128, num_neurons=[512], **moe_ref.MOE_KWARGS["encoder"]).train()
    own = m.state_dict()
    for key, v in sd.items():
        own[key[len(pre):]].copy_(torch.from_numpy(v))
    m.to(DEV)
    experts = moe_ref.experts_of(sd, pre)
    want, p, sel_ref, g_ref = moe_ref.sublayer(fx["x"], sd[pre + "w_gate"], experts, 2, sd[pre + "w_noise"], fx["randn"])
    assert np.array_equal(sel_ref, fx["gate_sel"])
    out, sel, g = m.sublayer(t(fx["x"]), noise=t(fx["randn"]), return_routing=True)
    assert_bits_equal(sel, sel_ref, "sel")
    assert_bits_equal(g, g_ref, "gates")
    assert_bits_equal(out, want, "output")
    np.testing.assert_allclose(out.cpu().numpy() - fx["x"], fx["y"], rtol=0, atol=1e-5)
    # fresh draws in training mode, none in eval mode
    a, b = m.sublayer(t(fx["x"])), m.sublayer(t(fx["x"]))
    assert not torch.equal(a, b)
    m.eval()
    a, b = m.sublayer(t(fx["x"])), m.sublayer(t(fx["x"]))
    assert torch.equal(a, b)
    assert_bits_equal(a, moe_ref.sublayer(fx["x"], sd[pre + "w_gate"], experts, 2)[0], "eval mode: the clean gate")


def test_expert_packs_follow_their_parameters():
    """The packed expert weights live in persistent buffers refreshed in place when a parameter changes."""
    from eam_rl4co_amd.policy import MoE

    torch.manual_seed(0)
    m = MoE(128, 128, num_neurons=[512], num_experts=2, k=1, noisy_gating=False).eval().to(DEV)
    x = torch.randn(40, 128, device=DEV)
    y0 = m.sublayer(x)
    pk = m.packed_experts()
    ptrs = {k: v.data_ptr() for k, v in pk.items()}
    assert m.packed_experts() is pk
    with torch.no_grad():
        m.experts[0].lins[1].bias.add_(1.0)             # with w_gate = 0 every row goes to expert 0
    y1 = m.sublayer(x)
    assert {k: v.data_ptr() for k, v in m.packed_experts().items()} == ptrs
    g = np.float32(1.0) / (np.float32(1.0) + np.float32(1e-6))
    np.testing.assert_allclose((y1 - y0).cpu().numpy(), np.full((40, 128), g, np.float32), rtol=0, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# whole rollouts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", moe_ref.ROLLOUT_FIXTURES)
def test_policy_rollout_bit_exact(name):
    from eam_rl4co_amd import _lib, ops

    fx, ref = moe_ref.reference(name)
    env_name = str(fx["env_name"])
    pol = make_policy(moe_ref.cfg_for(fx), fx)
    env, td = make_td(env_name, fx["locs"], fx.get("demand"))
    kw = call_kwargs(fx)
    B, M = fx["locs"].shape[:2]
    S = max(int(fx["num_starts"]), 1)
    # per layer, through the module: routing and embeddings
    with torch.no_grad():
        h = pol.encoder.init_embedding(td)
        for li, layer in enumerate(pol.encoder.net.layers):
            h = layer(h)
            assert_bits_equal(h, ref["layers"][li][0], f"embeddings after layer {li}")
    out = pol(td, env, phase="test", **kw)
    assert_bits_equal(out["actions"], ref["actions"], "tours")
    assert_bits_equal(out["actions"], fx["actions"], "tours against the reference")
    assert_bits_equal(out["log_likelihood"], ref["logp_steps"], "per-step log-probs")
    assert_bits_equal(out["reward"], ref["reward"], "reward")
    np.testing.assert_allclose(out["reward"].cpu().numpy(), fx["reward"], rtol=1e-6)
    np.testing.assert_allclose(out["log_likelihood"].cpu().numpy(), fx["logp_steps"], rtol=0, atol=1e-5)
    cs = _lib.Cache()
    cs.B, cs.M, cs.E, cs.H, cs.ld = B, M, 128, 8, (5 * 128 if M <= 128 else 128)
    kernel = ops.rollout_kernel(env_name, cs, B * S, ref["actions"].shape[1] - (1 if S > 1 else 0))
    print(f"MOEG {name}: rollout kernel {kernel}, M = {M}")
    if "pomo" in name:
        assert kernel == "ms_mfma", "the POMO case runs through the start-sharing kernel"
    if name == "moe_cvrp112_greedy":
        assert M == 113 and not ops.encoder_fused_supported(M, 128, 8, 512, 3)     # the large-graph attention path's first size


def test_graphed_rollout_equals_eager_on_other_routings():
    """A captured rollout replayed on other batches: the grids depend on (rows, k, num_experts) only, so the replay serves
    whatever routing the new batch has.  Instance norm centres every instance's embeddings, so a random gate spreads the
    rows over the experts and the loads move with the batch."""
    import eam_rl4co_amd as ea

    torch.manual_seed(5)
    pol = ea.AttentionModelPolicy(env_name="tsp", normalization="instance", moe_kwargs=moe_ref.MOE_KWARGS).eval()
    with torch.no_grad():
        for layer in pol.encoder.net.layers:
            layer[2].module.w_gate.normal_(0, 0.3)
    pol.to(DEV)
    env = ea.get_env("tsp", generator_params=dict(num_loc=20), seed=3)
    tds = [env.reset(batch_size=[8]).to(DEV) for _ in range(3)]
    g = ea.GraphedRollout(pol, env, tds[0], decode_type="greedy")
    m = pol.encoder.net.layers[0][2].module
    inner, loads = m.sublayer, []

    def recording(h, bn=None, noise=None, return_routing=False):          # (eager calls only: installed after the capture)
        out, sel, gates = inner(h, bn=bn, noise=noise, return_routing=True)
        loads.append(torch.bincount(sel.reshape(-1).long(), minlength=4).tolist())
        return (out, sel, gates) if return_routing else out

    for td in tds + [tds[0]]:
        a = g(td)
        m.sublayer = recording
        try:
            b = pol(td.clone(), env, phase="test", decode_type="greedy")
        finally:
            del m.sublayer
        assert_bits_equal(a["actions"], b["actions"], "actions")
        assert_bits_equal(a["reward"], b["reward"], "reward")
        assert_bits_equal(a["log_likelihood"], b["log_likelihood"], "ll")
    print("MOEG graphed replays, layer 0 rows per expert:", loads)
    assert len(loads) == 4 and loads[0] == loads[3]
    assert loads[0] != loads[1] and loads[0] != loads[2], "the other batches route differently"


def test_single_expert_equals_the_plain_policy():
    """k = num_experts = 1 with the expert copied from a plain FFN: the gate is 1 / (1 + 1e-6), so the policy's tours are the
    plain policy's on the layer-by-layer path and its log-likelihoods are close."""
    from test_gpu_parity import make_policy as make_plain

    fx = golden("cvrp20_greedy")
    plain = make_plain("am_cvrp")
    import eam_rl4co_amd as ea

    moe = ea.AttentionModelPolicy(env_name="cvrp", moe_kwargs={"encoder": dict(moe_ref.MOE_KWARGS["encoder"], num_experts=1, k=1),
                                                               "decoder": None}).eval().to(DEV)
    sd, own = plain.state_dict(), moe.state_dict()
    for key, v in sd.items():
        own[key.replace(".2.module.lins.", ".2.module.experts.0.lins.")].copy_(v)
    assert not any(own[k].any() for k in own if k.endswith("w_gate"))
    env, td = make_td("cvrp", fx["locs"], fx.get("demand"))
    old = os.environ.get("EAMRL_FUSED_ENCODER")
    os.environ["EAMRL_FUSED_ENCODER"] = "0"
    try:
        a = plain(td, env, phase="test", decode_type="greedy")
        b = moe(td, env, phase="test", decode_type="greedy")
    finally:
        if old is None:
            del os.environ["EAMRL_FUSED_ENCODER"]
        else:
            os.environ["EAMRL_FUSED_ENCODER"] = old
    assert_bits_equal(b["actions"], a["actions"], "tours")
    assert_bits_equal(b["actions"], fx["actions"], "tours against the reference's plain policy")
    np.testing.assert_allclose(b["log_likelihood"].cpu().numpy(), a["log_likelihood"].cpu().numpy(), rtol=0, atol=1e-4)


@pytest.mark.parametrize("env_name", ["tsp", "cvrp", "sdvrp", "pctsp", "spctsp", "op", "cvrptw", "pdp"])
def test_every_env_family_rolls_out(env_name):
    """The sublayer is env-agnostic: every env the plain policy serves, greedy and multistart sampling, valid finite tours."""
    import eam_rl4co_amd as ea

    torch.manual_seed(5)
    pol = ea.AttentionModelPolicy(env_name=env_name, moe_kwargs=moe_ref.MOE_KWARGS).eval()
    with torch.no_grad():
        for layer in pol.encoder.net.layers:
            layer[2].module.w_gate.normal_(0, 0.1)
    pol.to(DEV)
    env = ea.get_env(env_name, generator_params=dict(num_loc=20), seed=11)
    td = env.reset(batch_size=[6]).to(DEV)
    out = pol(td.clone(), env, phase="test", decode_type="greedy")
    assert torch.isfinite(out["reward"]).all() and torch.isfinite(out["log_likelihood"]).all()
    env.check_solution_validity(pol._last_td, out["actions"])
    np.testing.assert_allclose(out["reward"].cpu().numpy(), env.get_reward(pol._last_td, out["actions"]).cpu().numpy(), rtol=1e-6)
    if env_name != "op":
        ms = pol(td.clone(), env, phase="test", decode_type="multistart_sampling", num_starts=4)
        assert ms["reward"].shape == (24,) and torch.isfinite(ms["reward"]).all()


def test_decoding_options_and_evaluators():
    import eam_rl4co_amd as ea
    from eam_rl4co_amd.eval import evaluate_policy

    fx = golden("moe_cvrp20_greedy")
    pol = make_policy("am_cvrp_moe", fx)
    env, td = make_td("cvrp", fx["locs"], fx["demand"])
    greedy = pol(td, env, phase="test", decode_type="greedy")
    for kw in (dict(decode_type="sampling", top_k=5), dict(decode_type="sampling", top_p=0.9),
               dict(decode_type="beam_search", beam_width=4), dict(decode_type="multistart_greedy", num_starts=5, select_best=True)):
        out = pol(td.clone(), env, phase="test", **kw)
        assert torch.isfinite(out["reward"]).all() and out["reward"].shape == greedy["reward"].shape, kw
    ev = pol(td, env, phase="test", actions=greedy["actions"])
    assert_bits_equal(ev["log_likelihood"], greedy["log_likelihood"], "evaluate vs greedy")
    ds = ea.get_env("cvrp", generator_params=dict(num_loc=20), seed=13).dataset(batch_size=[8], phase="test")
    for method in ("greedy", "sampling", "augment_dihedral_8"):
        res = evaluate_policy(ea.get_env("cvrp", generator_params=dict(num_loc=20), seed=13), pol, ds, method=method, samples=4)
        assert res["rewards"].shape == (8,) and torch.isfinite(res["rewards"]).all(), method


# ---------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------
def test_reinforce_step_matches_the_reference_gradients():
    """One REINFORCE step (no baseline) in train() mode with noisy_gating off against the step recorded from the reference: tours,
    reward, log-likelihood, loss, every parameter's gradient and the batch norms' running statistics, held to the criterion of
    tests/test_gpu_polynet.py::test_poppy_step_matches_the_reference_gradients (1e-4 of the largest reference entry)."""
    from eam_rl4co_amd import train

    fx = golden("train_moe_cvrp20")
    pol = make_policy("am_cvrp_moe", fx, moe_kwargs={"encoder": dict(moe_ref.MOE_KWARGS["encoder"], noisy_gating=False),
                                                     "decoder": None}).train()
    env, td = make_td("cvrp", fx["locs"], fx["demand"])
    assert train.graph_encoder_equals_native(pol, td), "an MoE policy's step runs the encoder once"
    out = train.reinforce_loss(pol, env, td, baseline="no", noise=t(fx["noise"]))
    assert np.array_equal(out["actions"].cpu().numpy(), fx["actions"]), "actions"
    np.testing.assert_allclose(out["reward"].cpu().numpy(), fx["reward"], rtol=1e-6)
    ll = out["log_likelihood"]
    assert ll.requires_grad and ll.grad_fn is not None
    np.testing.assert_allclose(ll.detach().cpu().numpy(), fx["logp_steps"].sum(1), rtol=2e-5, atol=2e-5)
    loss = out["loss"]
    print(f"MOET train_moe_cvrp20: loss {float(loss.detach()):.8f} reference {float(fx['loss']):.8f}")
    np.testing.assert_allclose(float(loss.detach()), float(fx["loss"]), rtol=2e-5)
    loss.backward()
    params = dict(pol.named_parameters())
    total_ref = float(np.sqrt((fx["grad_norms"] ** 2).sum()))
    worst = 0.0
    for key, ref_norm in zip(fx["grad_names"], fx["grad_norms"]):
        g = params[str(key)].grad
        got = 0.0 if g is None else float(g.double().norm())
        worst = max(worst, abs(got - ref_norm) / max(ref_norm, 1e-3 * total_ref))
    print(f"MOET train_moe_cvrp20: largest relative gradient-norm difference {worst:.3e}")
    for key, ref_norm in zip(fx["grad_names"], fx["grad_norms"]):
        g = params[str(key)].grad
        got = 0.0 if g is None else float(g.double().norm())
        assert abs(got - ref_norm) <= 1e-4 * max(ref_norm, 1e-3 * total_ref) + 1e-7, (str(key), got, ref_norm)
        if "grad__" + str(key) in fx and g is not None:
            ref = fx["grad__" + str(key)]
            np.testing.assert_allclose(g.cpu().numpy(), ref, rtol=0, atol=1e-4 * max(float(np.abs(ref).max()), 1e-3 * total_ref),
                                       err_msg=str(key))
    assert float(params["encoder.net.layers.0.2.module.w_gate"].grad.abs().sum()) > 0
    g = params["encoder.net.layers.0.2.module.w_noise"].grad
    assert g is None or not g.any()
    bufs = dict(pol.named_buffers())        # the single pass keeps the running statistics, once
    for key in fx:
        if key.startswith("buf__"):
            np.testing.assert_allclose(bufs[key[5:]].cpu().numpy(), fx[key], rtol=1e-5, atol=1e-6, err_msg=key)
    assert int(bufs["encoder.net.layers.0.1.normalizer.num_batches_tracked"]) == 1


@pytest.mark.parametrize("cfg", ["am_cvrp_moe", "pomo_cvrp_moe"])
def test_noisy_step_runs_one_encoder_pass(cfg, monkeypatch):
    """With noisy gating the rollout and the gradient must see the same draw.  The re-evaluation is made to run its own
    forward (EAMRL_REEVAL_FORWARD=1) on the step's graph: its log-likelihood equals the rollout's within the bound of the
    reference-gradient tests -- with a second encoder pass (other noise, other routing) it would be another network's."""
    from eam_rl4co_amd import train

    fx = golden("moe_cvrp20_sampling")
    pol = make_policy(cfg).train()
    env, td = make_td("cvrp", fx["locs"], fx["demand"])
    seen = []
    orig = train.evaluate_log_likelihood

    def recording(*a, **kw):
        res = orig(*a, **kw)
        seen.append(res[0] if isinstance(res, tuple) else res)
        return res

    monkeypatch.setattr(train, "evaluate_log_likelihood", recording)
    monkeypatch.setenv("EAMRL_REEVAL_FORWARD", "1")
    torch.manual_seed(3)
    S = 4 if cfg.startswith("pomo") else 0
    out = train.reinforce_loss(pol, env, td, baseline="shared" if S else "mean", num_starts=S)
    assert len(seen) == 1
    native = out["log_likelihood"].detach().cpu().numpy()
    again = seen[0].detach().sum(1).cpu().numpy()
    print(f"MOET {cfg}: |rollout ll - re-evaluation ll| max {np.abs(native - again).max():.3e}")
    np.testing.assert_allclose(again, native, rtol=2e-5, atol=2e-5)
    out["loss"].backward()
    for li in range(len(pol.encoder.net.layers)):
        for nm in ("w_noise", "w_gate", "experts.0.lins.0.weight"):
            g = dict(pol.named_parameters())[f"encoder.net.layers.{li}.2.module.{nm}"].grad
            assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0, (li, nm)
    # and a second step draws other noise
    torch.manual_seed(4)
    out2 = train.reinforce_loss(pol, env, td, baseline="shared" if S else "mean", num_starts=S)
    assert not torch.equal(out2["log_likelihood"].detach(), out["log_likelihood"].detach())


def test_policy_gradient_step_moves_the_gate():
    """PolicyGradientStep works unchanged on an MoE policy: one optimizer step moves the gate."""
    from eam_rl4co_amd import train

    fx = golden("moe_cvrp20_sampling")
    pol = make_policy("am_cvrp_moe").train()
    env, td = make_td("cvrp", fx["locs"], fx["demand"])
    before = pol.encoder.net.layers[0][2].module.w_gate.detach().clone()
    step = train.PolicyGradientStep(pol, env, baseline="mean", lr=1e-3)
    torch.manual_seed(0)
    res = step(td)
    assert np.isfinite(float(res["loss"]))
    assert not torch.equal(pol.encoder.net.layers[0][2].module.w_gate.detach(), before)
    pol.eval()
    out = pol(td, env, phase="test", decode_type="greedy")          # the refreshed packs serve the next rollout
    assert torch.isfinite(out["reward"]).all()
