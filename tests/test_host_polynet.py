"""Host (no GPU): the PolyNet policy's contract, its weight constants, its loss, what it refuses, and the float64 restatement
tests/polynet_ref.py against the per-step log-probs recorded from the reference (tests/golden/make_golden_polynet.py).

Bound of the restatement test: the recorded log-probs are the reference's float32 ones.  A logit is a 128-term product sum behind a
384-term MLP and a 128-term projection, clipped to |10|; with u = 2^-24 and errors adding like a random walk that is about
10 * u * sqrt(128 + 384 + 128) = 1.5e-5 on the logit scale, which the log-softmax passes on at most once more: 2e-5, the tolerance
the rollout fixtures' log-likelihoods carry elsewhere in this suite.  Measured here: 9.3e-7 .. 3.1e-6 (the largest at polynet_tsp100_k128_s128_greedy).
"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

import polynet_ref as pr
from _util import golden

CONFIGS = [(env_name, k) for env_name in ("tsp", "cvrp") for k in (1, 2, 5, 8, 128)]


def make_policy(env_name="tsp", k=5, **kw):
    import eam_rl4co_amd as ea

    pol = ea.PolyNetPolicy(k=k, env_name=env_name, **kw).eval()
    sd = pol.state_dict()
    for key, v in pr.weights(env_name, k).items():
        sd[key].copy_(torch.from_numpy(v))
    return pol


def cpu_td(env_name="tsp", num_loc=20, batch=2):
    import eam_rl4co_amd as ea

    env = ea.get_env(env_name, generator_params=dict(num_loc=num_loc))
    torch.manual_seed(3)
    return env, env.reset(batch_size=[batch])


@pytest.mark.parametrize("env_name,k", CONFIGS)
def test_state_dict_contract(env_name, k):
    import eam_rl4co_amd as ea

    sd = ea.PolyNetPolicy(k=k, env_name=env_name).state_dict()
    got = [[key, list(v.shape), str(v.dtype).replace("torch.", "")] for key, v in sd.items()]
    assert got == pr.CONTRACT[f"polynet_{env_name}_k{k}"]
    for key in ("decoder.pointer.binary_vectors", "decoder.pointer.poly_layer_1.weight", "decoder.pointer.poly_layer_1.bias",
                "decoder.pointer.poly_layer_2.weight", "decoder.pointer.poly_layer_2.bias", "decoder.pointer.project_out.weight"):
        assert key in sd


def test_defaults_follow_the_reference():
    import eam_rl4co_amd as ea

    pol = ea.PolyNetPolicy(k=4)
    assert (pol.train_decode_type, pol.val_decode_type, pol.test_decode_type) == ("sampling",) * 3
    assert len(pol.encoder.net.layers) == 6 and pol.temperature == 1.0 and pol.tanh_clipping == 10.0
    assert isinstance(pol.decoder, ea.PolyNetDecoder) and isinstance(pol.decoder.pointer, ea.PolyNetAttention)
    assert not pol.decoder.pointer.binary_vectors.requires_grad
    assert isinstance(pol.encoder, ea.AttentionModelEncoder)


@pytest.mark.parametrize("k", [2, 5, 8, 128])
def test_binary_vectors(k):
    import eam_rl4co_amd as ea

    dz = math.ceil(math.log2(k))
    table = np.array(list(itertools.product([0, 1], repeat=dz))[:k], np.float32)
    got = ea.PolyNetAttention(k, 128, 256, 8).binary_vectors.numpy()
    assert got.shape == (k, dz) and np.array_equal(got, table)


@pytest.mark.parametrize("name", pr.ROLLOUT_FIXTURES)
def test_restatement_reproduces_the_recorded_log_probs(name):
    fx, _, lp = pr.reference(name)
    # the recorder's condition on the fixture; the one fixture with 25 600 decisions cannot meet it and stores what it has
    # (tests/golden/make_golden_polynet.py explains the arithmetic)
    assert (float(fx["min_top2_gap"]) >= 1e-4 or str(fx["decode_type"]) == "evaluate"
            or (name == "polynet_tsp100_k128_s128_greedy" and float(fx["min_top2_gap"]) >= 1.9e-5))
    assert lp.shape == fx["logp_steps"].shape
    err = float(np.abs(lp - fx["logp_steps"].astype(np.float64)).max())
    print(f"POLYH {name}: restatement against the recorded float32 log-probs {err:.3e}")
    assert err <= 2e-5


def test_pack_mfma_a_is_the_documented_order():
    from eam_rl4co_amd import ops

    rng = np.random.default_rng(0)
    for N, K in ((16, 16), (32, 48), (128, 128), (256, 128), (128, 256)):
        W = rng.standard_normal((N, K)).astype(np.float32)
        want = np.empty(N * K, np.float32)
        for T, q, l, i in itertools.product(range(N // 16), range(K // 16), range(64), range(4)):
            want[4 * ((T * (K // 16) + q) * 64 + l) + i] = W[16 * T + l % 16, 16 * q + 4 * i + l // 16]
        assert np.array_equal(ops.pack_mfma_a(torch.from_numpy(W)).numpy(), want)


@pytest.mark.parametrize("k", [1, 5, 128])
def test_operands_equal_their_float64_definitions(k):
    from eam_rl4co_amd import ops

    pol = make_policy("tsp", k)
    sd = {key: v.numpy().copy() for key, v in pol.state_dict().items()}
    op = pol.decoder.poly_operands()
    assert op is pol.decoder.poly_operands()                 # cached until a parameter changes
    W1, b1 = sd["decoder.pointer.poly_layer_1.weight"], sd["decoder.pointer.poly_layer_1.bias"]
    ctab = (pr.binary_vectors(k).astype(np.float64) @ W1[:, 128:].astype(np.float64).T + b1.astype(np.float64)).astype(np.float32)
    assert op["ctab"].shape == (k, 256) and (op["k"], op["P"]) == (k, 256)
    np.testing.assert_array_max_ulp(op["ctab"].numpy(), ctab, maxulp=1)
    assert torch.equal(op["W1"], ops.pack_mfma_a(torch.from_numpy(np.ascontiguousarray(W1[:, :128]))))
    assert torch.equal(op["Wout"], ops.pack_mfma_a(torch.from_numpy(sd["decoder.pointer.project_out.weight"])))
    assert torch.equal(op["W2"], ops.pack_mfma_a(torch.from_numpy(sd["decoder.pointer.poly_layer_2.weight"])))
    assert np.array_equal(op["b2"].numpy(), sd["decoder.pointer.poly_layer_2.bias"])
    with torch.no_grad():
        pol.decoder.pointer.poly_layer_2.bias.add_(1.0)      # an in-place update (optimizer step) is seen
    assert np.array_equal(pol.decoder.poly_operands()["b2"].numpy(), sd["decoder.pointer.poly_layer_2.bias"] + 1.0)


def test_polynet_loss_is_the_reference_formula():
    """zoo/polynet/model.py:224-231 with the shared baseline, restated line by line and differentiated by autograd."""
    from eam_rl4co_amd import train

    torch.manual_seed(11)
    reward = -torch.rand(6, 9, dtype=torch.float64) * 5
    reward[2, 4] = reward[2, 1] = reward[2].max() + 0.5      # two equal best rollouts: one of them carries the gradient
    ll_a = torch.randn(6, 9, dtype=torch.float64, requires_grad=True)
    ll_b = ll_a.detach().clone().requires_grad_(True)
    bl_val = reward.mean(dim=1, keepdims=True)
    best_idx = (-reward).argsort(1).argsort(1)
    mask = best_idx < 1
    want = -((reward - bl_val) * ll_a * mask).mean()
    got = train.polynet_loss(reward, ll_b)
    assert float(got.detach()) == float(want.detach())
    want.backward()
    got.backward()
    assert torch.equal(ll_a.grad, ll_b.grad)
    assert int((ll_b.grad != 0).sum()) == 6 and (ll_b.grad != 0).sum(1).eq(1).all()


def test_unsupported_constructions_raise():
    import eam_rl4co_amd as ea

    with pytest.raises(NotImplementedError, match="MatNet"):
        ea.PolyNetPolicy(k=4, encoder_type="MatNet")
    with pytest.raises(NotImplementedError, match="MatNet"):
        ea.PolyNetDecoder(k=4, encoder_type="MatNet")
    with pytest.raises(NotImplementedError, match="poly_layer_dim"):
        ea.PolyNetPolicy(k=4, poly_layer_dim=128)
    for env_name in ("sdvrp", "pdp", "op"):
        with pytest.raises(NotImplementedError, match="'tsp' and 'cvrp'"):
            ea.PolyNetPolicy(k=4, env_name=env_name)
    with pytest.raises(NotImplementedError, match="stand-alone"):
        ea.PolyNetAttention(4, 128, 256, 8)(None, None, None, None)


@pytest.mark.parametrize("kw,match", [
    (dict(), "one row per instance"),
    (dict(num_starts=1, multisample=True), "one row per instance"),
    (dict(num_starts=4, multisample=True, top_k=5), "top-k"),
    (dict(num_starts=4, multisample=True, top_p=0.9), "top-k"),
    (dict(num_starts=4, multisample=True, store_all_logp=True), "store_all_logp"),
    (dict(num_starts=4, multisample=True, return_entropy=True), "store_all_logp"),
    (dict(num_starts=4, multisample=True, decode_type="beam_search"), "beam search"),
    (dict(num_starts=4, multisample=True, select_best=True), "select_best"),
])
def test_unsupported_rollouts_raise_before_any_device_work(kw, match):
    pol = make_policy("tsp", 4)
    env, td = cpu_td()
    with pytest.raises(NotImplementedError, match=match):
        pol(td, env, phase="test", **kw)


def test_graphs_above_112_nodes_and_capture_raise():
    import eam_rl4co_amd as ea

    pol = make_policy("tsp", 4)
    env, td = cpu_td(num_loc=113)
    with pytest.raises(NotImplementedError, match="112 nodes"):
        pol(td, env, phase="test", num_starts=4, multisample=True)
    env, td = cpu_td()
    with pytest.raises(NotImplementedError, match="PolyNet"):
        ea.GraphedRollout(pol, env, td, num_starts=4, multisample=True)


def test_cpu_tensordict_has_no_fallback():
    pol = make_policy("tsp", 4)
    env, td = cpu_td()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pol(td, env, phase="test", num_starts=4, multisample=True, decode_type="greedy")


def test_native_reeval_is_not_claimed():
    from eam_rl4co_amd import train

    assert train.native_reeval_supported(make_policy("tsp", 4), 20) is False


def test_plain_checkpoint_loads_non_strictly_and_polynet_checkpoint_strictly():
    import eam_rl4co_amd as ea

    am = ea.AttentionModelPolicy(env_name="tsp", num_encoder_layers=6, normalization="instance")
    pol = ea.PolyNetPolicy(k=4)
    res = ea.load_reference_checkpoint(pol, {"state_dict": {"policy." + k: v for k, v in am.state_dict().items()}}, strict=False)
    assert not res.unexpected_keys
    assert sorted(res.missing_keys) == sorted("decoder.pointer." + n for n in (
        "binary_vectors", "poly_layer_1.weight", "poly_layer_1.bias", "poly_layer_2.weight", "poly_layer_2.bias"))
    assert torch.equal(pol.decoder.pointer.project_out.weight, am.decoder.pointer.project_out.weight)
    src = make_policy("tsp", 4)
    ea.load_reference_checkpoint(pol, {"state_dict": {"policy." + k: v for k, v in src.state_dict().items()}})
    for (ka, va), (kb, vb) in zip(pol.state_dict().items(), src.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)


def test_abi_refuses_unsupported_shapes_before_any_launch():
    from eam_rl4co_amd import _lib

    lib = _lib.load()

    def cache(M=20, B=2, E=128, H=8):
        c = _lib.Cache()
        c.ld, c.B, c.M, c.E, c.H = 6 * E, B, M, E, H
        return c

    sup = lambda env, c, R: lib.eamrl_rollout_polynet_supported(env, C.byref(c), R)
    assert sup(_lib.ENV_TSP, cache(), 8) == 1 and sup(_lib.ENV_CVRP, cache(21), 16) == 1
    assert sup(_lib.ENV_TSP, cache(112), 2 * 800) == 1          # more than 128 rows per instance: split into launches
    assert sup(_lib.ENV_TSP, cache(113), 8) == 0 and sup(_lib.ENV_TSP, cache(), 2) == 0 and sup(_lib.ENV_TSP, cache(), 7) == 0
    assert sup(_lib.ENV_TSP, cache(E=64), 8) == 0 and sup(_lib.ENV_TSP, cache(H=4), 8) == 0
    for env in (_lib.ENV_SDVRP, _lib.ENV_PCTSP, _lib.ENV_OP, _lib.ENV_CVRPTW, _lib.ENV_PDP):
        assert sup(env, cache(21), 8) == 0
    assert lib.eamrl_am_rollout_polynet(_lib.ENV_TSP, None, None, None, 8, 0, None, None, 0, 10.0, 1.0, 20, None, None, None,
                                        None, None) == -1
    assert b"eamrl_am_rollout_polynet" in lib.eamrl_last_error()
    assert lib.eamrl_am_rollout_polynet_seeded(_lib.ENV_TSP, None, None, None, 8, 1, None, 10.0, 1.0, 20, None, None, None, None,
                                               None) == -1
    assert b"eamrl_am_rollout_polynet_seeded" in lib.eamrl_last_error()
