"""CPU: the opt-in 16-bit encoder's host side -- the float64 emulation of its numeric contract (checked against the fp32
oracle with rounding switched off) and AttentionModelPolicy's `precision` setting."""
import copy

import numpy as np
import pytest
import torch

import precision_emulation as emu
from _util import CONTRACT, golden_weights, instance_from_td


# am_cvrptw: its time-window features drive the embeddings to |h| ~ 350, where the fp32 oracle itself is ~5e-6 (measured
# 4.8e-6) away from float64; every other config stays below 1e-6
@pytest.mark.parametrize("cfg,env_name,N,B,tol", [("am_tsp", "tsp", 20, 3, 1e-6), ("am_cvrp", "cvrp", 33, 2, 1e-6),
                                                  ("pomo_tsp", "tsp", 17, 2, 1e-6), ("pomo_cvrp", "cvrp", 20, 2, 1e-6),
                                                  ("am_sdvrp", "sdvrp", 15, 2, 1e-6), ("am_op", "op", 21, 2, 1e-6),
                                                  ("am_pctsp", "pctsp", 12, 2, 1e-6), ("am_cvrptw", "cvrptw", 10, 2, 1e-5)])
def test_emulation_without_rounding_matches_oracle(oracle, cfg, env_name, N, B, tol):
    import eam_rl4co_amd as ea

    env = ea.get_env(env_name, generator_params=dict(num_loc=N), seed=N)
    torch.manual_seed(N)
    td = env.reset(batch_size=[B])
    sd = golden_weights(cfg)
    init_o, h_o = oracle.encode(sd, env_name, td["locs"].numpy(), instance_from_td(env_name, td))
    h_e = emu.encode(sd, init_o)
    assert emu.rel_err(h_e, h_o) <= tol
    c_o = oracle.precompute(sd, env_name, h_o, use_graph_context=not cfg.startswith("pomo"))
    c_e = emu.precompute(sd, env_name, h_o, use_graph_context=not cfg.startswith("pomo"))
    for name in ("K", "V", "L", "Pa", "Pb", "Lp", "gctx"):
        if c_o[name] is None:
            assert c_e[name] is None, name
            continue
        assert emu.rel_err(c_e[name], c_o[name]) <= tol, name


def test_emulation_rounding():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.0e38, 7.0e4, np.nan])
    b = emu.round_bf16(x)
    assert b[0] == 1.0 and b[1] == 1.0 and b[2] == 1.0 + 2.0 ** -6        # ties to even
    assert np.isfinite(b[3]) and np.isnan(b[5])
    h = emu.round_fp16(x)
    assert h[1] == 1.0 + 2.0 ** -8 and np.isinf(h[4])                     # fp16: 10 mantissa bits, max 65504
    ref = torch.tensor(x, dtype=torch.float32)
    np.testing.assert_array_equal(b[:5], ref.to(torch.bfloat16).double().numpy()[:5])
    np.testing.assert_array_equal(h[:5], ref.to(torch.float16).double().numpy()[:5])


def test_precision_setting_validates_and_defaults():
    import eam_rl4co_amd as ea

    pol = ea.AttentionModelPolicy(env_name="tsp")
    assert pol.precision == "32-true" and pol.encoder.net.dtype16 is None
    for name, dt in (("16-mixed", torch.float16), ("bf16-mixed", torch.bfloat16), ("32-true", None)):
        pol.precision = name
        assert pol.precision == name and pol.encoder.net.dtype16 is dt
    assert ea.AttentionModelPolicy(env_name="cvrp", precision="bf16-mixed").encoder.net.dtype16 is torch.bfloat16
    for bad in ("16", "bf16", "fp16", "32", "64-true", "16-true", None):
        with pytest.raises(ValueError):
            ea.AttentionModelPolicy(env_name="tsp", precision=bad)
        with pytest.raises(ValueError):
            pol.precision = bad
    assert pol.precision == "32-true"


@pytest.mark.parametrize("precision", ["32-true", "16-mixed", "bf16-mixed"])
def test_precision_keeps_state_dict_contract(precision):
    import eam_rl4co_amd as ea

    sd = ea.AttentionModelPolicy(env_name="tsp", precision=precision).state_dict()
    assert list(sd.keys()) == [k for k, _, _ in CONTRACT["am_tsp"]]
    pol = ea.AttentionModelPolicy(env_name="tsp")
    pol.load_state_dict(sd)
    pol.precision = precision
    assert list(pol.state_dict().keys()) == list(sd.keys())


def test_precision_survives_deepcopy():
    import eam_rl4co_amd as ea

    pol = ea.AttentionModelPolicy(env_name="cvrp", precision="16-mixed")
    twin = copy.deepcopy(pol)       # what the reference's RolloutBaseline does with the policy
    assert twin.precision == "16-mixed" and twin.encoder.net.dtype16 is torch.float16
    twin.precision = "bf16-mixed"
    assert pol.precision == "16-mixed" and pol.encoder.net.dtype16 is torch.float16
