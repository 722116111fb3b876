"""GPU: the opt-in 16-bit fused encoder (eamrl_encoder_fused16, AttentionModelPolicy(precision="16-mixed" / "bf16-mixed")).

No bit-exact oracle exists for 16-bit MFMA (the accumulation order inside one instruction is not documented), so the
embeddings and the decoder cache are held against the float64 emulation of the contract (tests/precision_emulation.py):
much closer to it than to the fp32 path, which pins the rounding points.  Everything around the encoder -- the init
embedding, the decode kernels, the fall-backs -- is held bit for bit."""
import os

import numpy as np
import pytest
import torch

import precision_emulation as emu
from _util import golden_weights
from test_gpu_parity import DEV, assert_bits_equal, make_policy

pytestmark = pytest.mark.gpu

PREC = {"bf16": "bf16-mixed", "fp16": "16-mixed"}
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
# relative Frobenius bounds from the unit round-offs (bf16 2^-8, fp16 2^-11).  Measured maxima of e16 on MI355X: AM configs
# bf16 1.9e-3, fp16 3.1e-4; POMO configs (6 layers, twice the rounding points) bf16 3.3e-3 (Lp of pomo_cvrp), fp16 3.5e-4,
# so the bf16 bound of the 6-layer configs is 5e-3
E16_MAX = {"bf16": 3e-3, "fp16": 5e-4}
E16_MAX_6_LAYERS = {"bf16": 5e-3, "fp16": 5e-4}
E32_MAX = {"bf16": 5e-2, "fp16": 1e-2}
# e32 / e16 floor.  Measured on MI355X over SHAPES (min .. max over the output tensors): AM configs (3 layers, batch norm)
# bf16 2.7 .. 17, fp16 1.55 .. 13 (lowest: Lp, two rounded products deep); POMO configs (6 layers, instance norm) 1.44 .. 2.8.
# am_pctsp bf16 sits at e16 ~ 1e-7, the fp32-vs-float64 floor.  e16 is larger elsewhere because where the kernel's fp32
# value and the emulation's float64 value straddle a rounding boundary of T they differ by one T ulp, and such elements
# spread through the later layers: e16 grows with the number of rounding points, so the floor is below the 4 first assumed.
E32_OVER_E16_MIN = 1.25

SHAPES = [
    ("am_tsp", "tsp", 5, 3), ("am_tsp", "tsp", 16, 2), ("am_tsp", "tsp", 17, 2), ("am_tsp", "tsp", 20, 7), ("am_tsp", "tsp", 32, 3),
    ("am_tsp", "tsp", 33, 3), ("am_tsp", "tsp", 50, 5), ("am_tsp", "tsp", 64, 2), ("am_tsp", "tsp", 65, 2), ("am_tsp", "tsp", 100, 9),
    ("am_tsp", "tsp", 112, 2), ("am_cvrp", "cvrp", 20, 4), ("am_cvrp", "cvrp", 100, 5), ("am_cvrp", "cvrp", 111, 2),
    ("pomo_tsp", "tsp", 20, 3), ("pomo_tsp", "tsp", 100, 4), ("pomo_cvrp", "cvrp", 50, 3), ("am_pctsp", "pctsp", 30, 2),
]


def _encode_with_cache(pol, td, dtype):
    B, M = td["action_mask"].shape
    with torch.no_grad():
        spec = pol.decoder._fused_cache_spec(B, M, DEV, dtype=dtype)
        h, init_h = pol.encoder(td, cache_spec=spec)
    assert spec["filled"]
    slots = {n: i for i, n in enumerate(["K", "V", "L", "Pa", "Pb", "Lp"] if pol.env_name == "tsp" else ["K", "V", "L", "Pa", "Lp"])}
    E = h.shape[-1]
    buf = spec["buf"].cpu().numpy()
    out = {n: buf[..., s * E:(s + 1) * E] for n, s in slots.items()}
    out["gctx"] = spec["gctx"].cpu().numpy() if spec.get("gctx") is not None else None
    out["emb"] = h.cpu().numpy()
    return out, init_h


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("cfg,env_name,N,B", SHAPES)
def test_fused16_embeddings_and_cache_follow_the_contract(cfg, env_name, N, B, kind):
    import eam_rl4co_amd as ea

    env = ea.get_env(env_name, generator_params=dict(num_loc=N), seed=N)
    torch.manual_seed(N * 31 + B)
    td = env.reset(batch_size=[B]).to(DEV)
    pol = make_policy(cfg)
    r32, init32 = _encode_with_cache(pol, td, None)
    pol.precision = PREC[kind]
    r16, init16 = _encode_with_cache(pol, td, DT[kind])
    assert_bits_equal(init16, init32, "init embeddings")
    sd = golden_weights(cfg)
    rnd = emu.ROUNDING[kind]
    h_e = emu.encode(sd, init32.cpu().numpy(), rnd)
    c_e = emu.precompute(sd, env_name, h_e, rnd, use_graph_context=not cfg.startswith("pomo"))
    c_e["emb"] = h_e
    report = []
    for name in ("emb", "K", "V", "L", "Pa", "Pb", "Lp", "gctx"):
        if name not in r16 or r16[name] is None:
            continue
        e16, e32 = emu.rel_err(r16[name], c_e[name]), emu.rel_err(r16[name], r32[name])
        report.append(f"{name}: e16={e16:.2e} e32={e32:.2e}")
        assert np.isfinite(r16[name]).all(), name
        assert e16 <= (E16_MAX_6_LAYERS if cfg.startswith("pomo") else E16_MAX)[kind], report
        assert 0 < e32 <= E32_MAX[kind], report
        assert e32 >= E32_OVER_E16_MIN * e16, report
    print(f"{cfg} N={N} {kind}: " + "; ".join(report))


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("kw", [dict(decode_type="greedy"), dict(decode_type="sampling"),
                                dict(decode_type="multistart_greedy", num_starts=8)])
def test_fused16_cache_through_step_api_equals_whole_rollout(kw, kind):
    """The decode kernels are the fp32 ones, unchanged: the 16-bit encoder's cache through the host-driven step loop
    gives the whole-rollout launch's tours, log-likelihoods and rewards bit for bit."""
    import eam_rl4co_amd as ea

    cfg, env_name, N, B = ("pomo_tsp", "tsp", 20, 4) if "multistart" in kw["decode_type"] else ("am_cvrp", "cvrp", 50, 6)
    env = ea.get_env(env_name, generator_params=dict(num_loc=N), seed=5)
    torch.manual_seed(7)
    td = env.reset(batch_size=[B]).to(DEV)
    pol = make_policy(cfg, precision=PREC[kind])
    extra = {}
    if kw["decode_type"] == "sampling":
        M = td["locs"].shape[1]
        extra["noise"] = torch.empty(B, 3 * M + 1, M, device=DEV).exponential_(1)
    a = pol(td.clone(), env, phase="test", **kw, **extra)
    os.environ["EAMRL_ENTROPY_STEPWISE"] = "1"
    try:
        b = pol(td.clone(), env, phase="test", return_entropy=True, **kw, **extra)
    finally:
        os.environ.pop("EAMRL_ENTROPY_STEPWISE", None)
    assert_bits_equal(a["actions"], b["actions"], "actions")
    assert_bits_equal(a["log_likelihood"], b["log_likelihood"], "log-likelihood")
    assert_bits_equal(a["reward"], b["reward"], "reward")


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("env_name", ["tsp", "cvrp", "sdvrp", "pctsp", "op", "cvrptw"])
@pytest.mark.parametrize("N", [20, 100])
def test_fused16_rollouts_are_valid(env_name, N, kind):
    import eam_rl4co_amd as ea

    env = ea.get_env(env_name, generator_params=dict(num_loc=N), seed=N + 11)
    torch.manual_seed(N)
    td = env.reset(batch_size=[16]).to(DEV)
    pol = make_policy("am_" + env_name, precision=PREC[kind])
    with torch.no_grad():
        out = pol(td.clone(), env, phase="test", decode_type="greedy")
        env.check_solution_validity(td, out["actions"])
        out2 = pol(td.clone(), env, phase="test", decode_type="greedy")
    assert torch.isfinite(out["reward"]).all()
    assert_bits_equal(out["actions"], out2["actions"], "two runs: actions")
    assert_bits_equal(out["log_likelihood"], out2["log_likelihood"], "two runs: log-likelihood")


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
def test_fused16_full_size_reward_matches_fp32(env_name, kind):
    """TSP-100 / CVRP-100 x 1024 greedy: mean reward within 1 % of the fp32 path (share of identical tours reported)."""
    import eam_rl4co_amd as ea

    env = ea.get_env(env_name, generator_params=dict(num_loc=100), seed=1234)
    torch.manual_seed(0)
    td = env.reset(batch_size=[1024]).to(DEV)
    pol = make_policy("am_" + env_name)
    with torch.no_grad():
        r32 = pol(td.clone(), env, phase="test", decode_type="greedy")
        pol.precision = PREC[kind]
        r16 = pol(td.clone(), env, phase="test", decode_type="greedy")
        r16b = pol(td.clone(), env, phase="test", decode_type="greedy")
    env.check_solution_validity(td, r16["actions"])
    m32, m16 = r32["reward"].mean().item(), r16["reward"].mean().item()
    same = (r32["actions"] == r16["actions"]).all(-1).float().mean().item() if r32["actions"].shape == r16["actions"].shape else 0.0
    print(f"{env_name}-100 x 1024 {kind}: reward fp32 {m32:.5f} 16-bit {m16:.5f} ({(m16 - m32) / abs(m32):+.3%}), "
          f"identical tours {same:.1%}")
    assert abs(m16 - m32) <= 0.01 * abs(m32)
    assert_bits_equal(r16["actions"], r16b["actions"], "two runs")
    assert_bits_equal(r16["reward"], r16b["reward"], "two runs")


def test_fused16_fallbacks_are_the_fp32_path():
    """Outside the fused kernel's coverage the fp32 path runs, bit for bit: M = 120, batch norm in training mode."""
    import eam_rl4co_amd as ea

    env = ea.get_env("tsp", generator_params=dict(num_loc=120), seed=3)
    td = env.reset(batch_size=[3]).to(DEV)
    pol = make_policy("am_tsp")
    with torch.no_grad():
        a = pol(td.clone(), env, phase="test", decode_type="greedy")
        pol.precision = "bf16-mixed"
        b = pol(td.clone(), env, phase="test", decode_type="greedy")
    assert_bits_equal(a["actions"], b["actions"], "M = 120 actions")
    assert_bits_equal(a["log_likelihood"], b["log_likelihood"], "M = 120 log-likelihood")

    env = ea.get_env("tsp", generator_params=dict(num_loc=20), seed=4)
    td = env.reset(batch_size=[8]).to(DEV)
    outs = []
    for prec in ("32-true", "16-mixed"):
        pol = make_policy("am_tsp", precision=prec).train()      # batch statistics (running stats updated alike)
        with torch.no_grad():
            outs.append(pol(td.clone(), env, phase="val", decode_type="greedy"))
    assert_bits_equal(outs[0]["actions"], outs[1]["actions"], "train-mode batch norm actions")
    assert_bits_equal(outs[0]["log_likelihood"], outs[1]["log_likelihood"], "train-mode batch norm log-likelihood")


def test_fused16_training_graph_raises():
    import eam_rl4co_amd as ea

    env = ea.get_env("tsp", generator_params=dict(num_loc=20), seed=5)
    td = env.reset(batch_size=[4]).to(DEV)
    pol = make_policy("am_tsp", precision="bf16-mixed")
    with pytest.raises(NotImplementedError):
        pol(td.clone(), env, phase="train")
    with torch.no_grad():           # the rollout baseline's greedy pass: no graph, 16-bit
        out = pol(td.clone(), env, phase="train", decode_type="greedy")
    assert out["log_likelihood"].grad_fn is None


def test_fused16_graphed_rollout_equals_eager_and_pins_precision():
    import eam_rl4co_amd as ea

    env = ea.get_env("tsp", generator_params=dict(num_loc=50), seed=6)
    td = env.reset(batch_size=[32]).to(DEV)
    pol = make_policy("am_tsp", precision="bf16-mixed")
    with torch.no_grad():
        eager = pol(td.clone(), env, phase="test", decode_type="greedy")
    g = ea.GraphedRollout(pol, env, td, decode_type="greedy")
    out = g(td)
    assert_bits_equal(out["actions"], eager["actions"], "graphed actions")
    assert_bits_equal(out["log_likelihood"], eager["log_likelihood"], "graphed log-likelihood")
    pol.precision = "32-true"
    with pytest.raises(RuntimeError, match="precision"):
        g(td)
    pol.precision = "bf16-mixed"
    assert_bits_equal(g(td)["actions"], eager["actions"], "graphed again")


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_fused16_follows_in_place_weight_updates(kind):
    """After optimizer.step the 16-bit packs are refreshed: the next rollout equals a fresh policy's with the new weights."""
    import eam_rl4co_amd as ea

    env = ea.get_env("cvrp", generator_params=dict(num_loc=30), seed=8)
    td = env.reset(batch_size=[8]).to(DEV)
    pol = make_policy("am_cvrp", precision=PREC[kind])
    with torch.no_grad():
        before = pol(td.clone(), env, phase="test", decode_type="greedy")
    opt = torch.optim.SGD(pol.parameters(), lr=1e-2)
    for p in pol.parameters():
        p.grad = torch.randn_like(p) * 0.5
    opt.step()
    with torch.no_grad():
        after = pol(td.clone(), env, phase="test", decode_type="greedy")
    fresh = ea.AttentionModelPolicy(env_name="cvrp", precision=PREC[kind]).eval().to(DEV)
    fresh.load_state_dict(pol.state_dict())
    with torch.no_grad():
        ref = fresh(td.clone(), env, phase="test", decode_type="greedy")
    assert_bits_equal(after["actions"], ref["actions"], "actions after the update")
    assert_bits_equal(after["log_likelihood"], ref["log_likelihood"], "log-likelihood after the update")
    assert not torch.equal(before["log_likelihood"], after["log_likelihood"])
