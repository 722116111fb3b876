"""CPU: the Heterogeneous Attention Model (HAM) policy for pickup and delivery -- what can be held without a GPU.

  - the restatement of the attention (tests/ham_ref.py) in float64 equals the outputs recorded from the reference's
    HeterogenousMHA module (run in float64) to 1e-12; measured 2.0e-15 at |out| <= 2.7
  - each deliberately wrong form (pair term dropped, same and other swapped, groups soft-maxed separately) misses that bound on
    every fixture, by five orders of magnitude and more
  - the module tree carries the reference's state-dict keys, shapes and dtypes; a checkpoint round-trips
  - the C ABI rejects a null pointer, an even node count and a graph above the stated bound before any launch
  - the constants of tests/ham_cases.py are what the CPU measures
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ham_cases as hc
import ham_ref
from _util import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND64 = 1e-12


@pytest.mark.parametrize("name", hc.MHA_FIXTURES)
def test_restatement_equals_the_recorded_module_outputs(name):
    fx = golden(name)
    x, w = torch.from_numpy(fx["x"]), hc.fixture_weights(fx)
    want = torch.from_numpy(fx["out"])
    assert want.dtype == torch.float64
    fig = float((ham_ref.module_forward(x, w, torch.float64) - want).abs().max())
    f32 = float((ham_ref.module_forward(x, w, torch.float32).double() - want).abs().max())
    print(f"HAMREF {name} float64 {fig:.3e} float32 {f32:.3e} |out| {float(want.abs().max()):.3f}")
    assert fig <= BOUND64
    assert f32 <= 1e-5                                  # float32 rounding, nothing else
    for wrong in ham_ref.WRONG:
        miss = float((ham_ref.module_forward(x, w, torch.float64, wrong=wrong) - want).abs().max())
        print(f"HAMREF {name} wrong={wrong} {miss:.3e}")
        assert miss > 1e5 * BOUND64, wrong


def test_restatement_gradient_is_the_gradient_of_the_restatement():
    """hetero_mha_backward against central differences of hetero_mha in float64 (M = 5, both roles, the depot's unused block)."""
    g = torch.Generator().manual_seed(11)
    proj = torch.randn(1, 5, 6 * hc.E, generator=g, dtype=torch.float64)
    dout = torch.randn(1, 5, hc.E, generator=g, dtype=torch.float64)
    _, d = ham_ref.hetero_mha_backward(proj, dout, hc.H)
    assert (d[:, 0, 3 * hc.E:] == 0).all()              # the depot's qpair | qsame | qother are never read
    f = lambda p: float((ham_ref.hetero_mha(p, hc.H) * dout).sum())
    idx = torch.randperm(proj.numel(), generator=g)[:40]
    for i in idx.tolist():
        e = torch.zeros(proj.numel(), dtype=torch.float64)
        e[i] = 1e-6
        e = e.view_as(proj)
        num = (f(proj + e) - f(proj - e)) / 2e-6
        assert abs(num - float(d.reshape(-1)[i])) <= 1e-7 * max(1.0, abs(num)), i


def _policy(cfg):
    import eam_rl4co_amd as ea

    return ea.HeterogeneousAttentionModelPolicy(**(hc.POMO if cfg == "pomo" else {}))


@pytest.mark.parametrize("cfg", ["am", "pomo"])
def test_state_dict_contract(cfg):
    pol = _policy(cfg)
    assert pol.env_name == "pdp"
    got = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in pol.state_dict().items()]
    assert got == hc.CONTRACT[cfg]
    keys = [k for k, _, _ in got]
    for name in ham_ref.WEIGHT_KEYS:
        assert f"encoder.layers.0.0.module.{name}" in keys
    assert pol.state_dict()["encoder.layers.0.0.module.W_query"].shape == (8, 128, 16)
    assert pol.state_dict()["encoder.layers.0.0.module.W_out"].shape == (8, 16, 128)
    assert {"encoder.layers.0.1.normalizer.weight", "encoder.layers.0.3.normalizer.bias", "encoder.layers.0.2.module.0.weight",
            "encoder.layers.0.2.module.2.bias", "encoder.init_embedding.init_embed_pick.weight"} <= set(keys)


def test_exports_and_reference_checkpoint_round_trip(tmp_path):
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import policy as pm

    assert issubclass(ea.HeterogeneousAttentionModelPolicy, ea.AttentionModelPolicy)
    for cls in ("HeterogenousMHA", "HeterogeneuousMHALayer", "GraphHeterogeneousAttentionEncoder"):      # the reference's spellings
        assert hasattr(pm, cls)
    assert isinstance(ea.HeterogeneousAttentionModelPolicy().encoder, ea.GraphHeterogeneousAttentionEncoder)
    src = _policy("am")
    sd = src.state_dict()
    for k, v in hc.weights("am").items():
        sd[k].copy_(torch.from_numpy(v))
    ckpt = {"state_dict": {**{"policy." + k: v for k, v in sd.items()}, "baseline.baseline.policy.junk": torch.zeros(1)}}
    path = tmp_path / "ham.ckpt"
    torch.save(ckpt, path)
    dst = _policy("am")
    res = ea.load_reference_checkpoint(dst, str(path))
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in dst.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError):                   # an AM checkpoint is not a HAM checkpoint
        ea.load_reference_checkpoint(_policy("am"), ea.AttentionModelPolicy(env_name="pdp").state_dict())
    with pytest.raises(NotImplementedError):            # 16-bit operands need the built-in GraphAttentionNetwork encoder
        ea.HeterogeneousAttentionModelPolicy(precision="bf16-mixed")


def test_packed_weights_follow_the_parameters():
    """HeterogenousMHA.packed(): [(h d), E] Linear weights of the [H, E, D] parameters, W_out.view(H D, E) transposed; repacked in
    place (same storage) when a parameter changes."""
    from eam_rl4co_amd.policy import HeterogenousMHA

    m = HeterogenousMHA(8, 128, 128)
    p = m.packed()
    x = torch.randn(5, 128)
    q_ref = torch.einsum("ne,hed->nhd", x, m.W_query.detach()).reshape(5, 128)
    assert torch.allclose(x @ p["qkv"][0:128].t(), q_ref, atol=1e-5)
    w3 = torch.einsum("ne,hed->nhd", x, m.W3_query.detach()).reshape(5, 128)
    assert torch.allclose(x @ p["pick"][256:384].t(), w3, atol=1e-5)
    assert torch.equal(p["out"].t(), m.W_out.detach().reshape(128, 128))
    ptrs = {k: v.data_ptr() for k, v in p.items()}
    assert {k: v.data_ptr() for k, v in m.packed().items()} == ptrs
    with torch.no_grad():
        m.W5_query.mul_(2.0)
    p2 = m.packed()
    assert {k: v.data_ptr() for k, v in p2.items()} == ptrs
    assert torch.equal(p2["deliv"][128:256], m.W5_query.detach().permute(0, 2, 1).reshape(128, 128))
    m.init_parameters()                                 # a re-initialisation moves the version counters too
    assert torch.equal(m.packed()["qkv"][0:128], m.W_query.detach().permute(0, 2, 1).reshape(128, 128))
    assert float(m.W_out.detach().abs().max()) <= 128 ** -0.5 and float(m.W_query.detach().abs().max()) <= 0.25


def test_even_graph_size_raises_the_reference_assertion_text():
    from eam_rl4co_amd import ops
    from eam_rl4co_amd.policy import HeterogenousMHA

    assert ops.ODD_NODES_MESSAGE.startswith("Graph size should have odd number of nodes due to pickup-delivery problem  ")
    assert ops.ODD_NODES_MESSAGE.endswith("   (n/2 pickup, n/2 delivery, 1 depot)") and len(ops.ODD_NODES_MESSAGE) == 147
    with pytest.raises(AssertionError, match="Graph size should have odd number of nodes"):
        HeterogenousMHA(8, 128, 128).project(torch.zeros(1, 4, 128))


def test_abi_declares_and_guards_the_entry_points():
    from eam_rl4co_amd import _lib
    from eam_rl4co_amd import build as b

    assert "hetero_attn.hip" in b.SOURCES
    with open(os.path.join(ROOT, "include", "eamrl.h")) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for fn in ("eamrl_hetero_mha", "eamrl_hetero_mha_supported", "eamrl_hetero_mha_backward", "eamrl_hetero_mha_backward_supported"):
        assert re.search(r"\bint\s+" + fn + r"\s*\(", code), fn
        assert fn in _lib.PROTOTYPES
    assert "zoo/ham/attention.py:53-488" in text
    defines = {k: int(v) for k, v in re.findall(r"#define\s+EAMRL_HETERO_MHA_(\w+)\s+(\d+)", text)}
    assert defines == {"MAX_NODES": hc.MAX_NODES, "BWD_MAX_NODES": hc.BWD_MAX_NODES}
    lib = _lib.load()
    assert lib.eamrl_version() == 101
    p, q, r = C.c_void_p(64), C.c_void_p(128), C.c_void_p(192)      # never dereferenced: every call is rejected before a launch

    def rejected(fn, *args):
        assert getattr(lib, fn)(*args) == -1
        msg = lib.eamrl_last_error()
        assert fn.encode() + b": requirement failed" in msg, msg

    for M in range(3, hc.MAX_NODES + 1, 2):
        assert lib.eamrl_hetero_mha_supported(M, 128, 8) == 1
        assert lib.eamrl_hetero_mha_backward_supported(M, 128, 8) == (1 if M <= hc.BWD_MAX_NODES else 0)
    for M, E, H in ((1, 128, 8), (20, 128, 8), (hc.MAX_NODES + 2, 128, 8), (21, 64, 8), (21, 128, 4), (-3, 128, 8)):
        assert lib.eamrl_hetero_mha_supported(M, E, H) == 0
        assert lib.eamrl_hetero_mha_backward_supported(M, E, H) == 0
        rejected("eamrl_hetero_mha", p, q, 2, M, E, H, None)
        rejected("eamrl_hetero_mha_backward", p, q, r, 2, M, E, H, None)
    rejected("eamrl_hetero_mha", None, q, 2, 21, 128, 8, None)
    rejected("eamrl_hetero_mha", p, None, 2, 21, 128, 8, None)
    rejected("eamrl_hetero_mha", p, q, -1, 21, 128, 8, None)
    rejected("eamrl_hetero_mha", C.c_void_p(68), q, 2, 21, 128, 8, None)            # float4 loads: 16-byte alignment
    for miss in range(3):
        args = [p, q, r]
        args[miss] = None
        rejected("eamrl_hetero_mha_backward", *args, 2, 21, 128, 8, None)
    rejected("eamrl_hetero_mha_backward", p, q, r, 2, hc.BWD_MAX_NODES + 2, 128, 8, None)
    assert lib.eamrl_hetero_mha(p, q, 0, 21, 128, 8, None) == 0                      # an empty batch launches nothing


@pytest.mark.parametrize("tag,cfg", [("batch", "am"), ("instance", "pomo")])
def test_encoder_restatement_and_the_embedding_bound(tag, cfg):
    """ham_ref.encoder against the embeddings recorded from the reference's encoder (float32): the float64 run is within the
    reference's own float32 rounding, and the float32 run's distance is the figure ham_cases.EMBED_F32_DISTANCE records (the GPU
    test allows MARGIN times it)."""
    fx = golden("ham_embed_pdp20")
    sd = {k: torch.from_numpy(v) for k, v in hc.weights(cfg).items()}
    locs = torch.from_numpy(fx["locs"])
    want = torch.from_numpy(fx["embeddings_" + tag]).double()
    layers = 6 if cfg == "pomo" else 3
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        h64, i64 = ham_ref.encoder(locs, sd, layers, tag, torch.float64)
        h32, _ = ham_ref.encoder(locs, sd, layers, tag, torch.float32)
    finally:
        torch.set_num_threads(threads)
    d64, d32 = float((h64 - want).abs().max()), float((h32.double() - want).abs().max())
    print(f"HAMENC {tag} float64 {d64:.3e} float32 {d32:.3e} |emb| {float(want.abs().max()):.3f}")
    assert float((i64 - torch.from_numpy(fx["init_embeds_" + tag]).double()).abs().max()) <= 5e-7
    assert d64 <= 5e-6
    rec = hc.EMBED_F32_DISTANCE[tag]
    assert 0.75 * rec <= d32 <= 1.25 * rec, (d32, rec)


def test_cases_cover_the_stated_shapes():
    Ms = {c["M"] for c in hc.CASES.values()}
    assert Ms == set(hc.FWD_SIZES) | {hc.MAX_NODES}
    assert {c["B"] for c in hc.CASES.values() if c["M"] in hc.FWD_SIZES and c["kind"] == "normal"} == {1, 3}
    assert hc.CASES[f"M{hc.MAX_NODES}_B2"]["B"] == 2
    assert all(hc.CASES[n]["M"] <= hc.BWD_MAX_NODES for n in hc.BWD_NAMES) and max(hc.CASES[n]["M"] for n in hc.BWD_NAMES) == 129
    assert {c["kind"] for c in hc.CASES.values()} == {"normal", "peak", "equal", "pair_high", "same_high"}
    op, r64, _ = hc.reference("M21_B2_peak")
    E, H, P = hc.E, hc.H, 10
    q, k = (op["proj"][..., i * E:(i + 1) * E].double().view(2, 21, H, 16) for i in (0, 1))
    s = 0.25 * torch.einsum("bihd,bjhd->bhij", q, k)
    rest = torch.cat((s[..., :P], s[..., P + 1:]), -1)
    assert float((s[..., P:P + 1] - rest).min()) > 55.0          # one key 60 (+- the noise) above the rest, in every row and head
    op, r64, _ = hc.reference("M21_B2_equal")
    v = op["proj"][..., 2 * E:3 * E].double()
    assert torch.allclose(r64["y"][:, 0], v.mean(1), atol=1e-12)          # the depot row: the plain mean of the values


@pytest.mark.parametrize("kind", ["pair_high", "same_high"])
def test_high_cases_need_the_maximum_over_all_groups(kind):
    """In these cases the pair score (every same-role score) of a non-depot row is about 100 above the row's general scores:
    exp(score - max over the general scores) is not a float32, so a maximum over the general group alone cannot pass them."""
    op, r64, r32 = hc.reference(f"M21_B2_{kind}")
    E, H, P, M = hc.E, hc.H, 10, 21
    part = lambda i: op["proj"][..., i * E:(i + 1) * E].double().view(2, M, H, 16)
    q, k = part(0), part(1)
    gen = 0.25 * torch.einsum("bihd,bjhd->bhij", q, k)[:, :, 1:]                       # non-depot rows
    if kind == "pair_high":
        partner = torch.cat((torch.arange(P + 1, M), torch.arange(1, P + 1)))
        high = 0.25 * (part(3)[:, 1:] * k[:, partner]).sum(-1).permute(0, 2, 1)[..., None]       # [B, H, M - 1, 1]
        v = op["proj"][..., 2 * E:3 * E].double()
        assert torch.allclose(r64["y"][:, 1:], v[:, partner], atol=1e-12)              # the output is the partner's value
    else:
        sx = 0.25 * torch.einsum("bihd,bjhd->bhij", part(4), k)[:, :, 1:]
        high = torch.cat((sx[:, :, :P, 1:P + 1], sx[:, :, P:, P + 1:]), 2)              # same-role blocks
    gap = float((high.amin(-1) - gen.amax(-1)).min())
    print(f"HAMCASE {kind}: smallest (high score - largest general score of the row) {gap:.2f}")
    assert gap > 89.0                                   # beyond log(float32 max) = 88.7
    assert all(torch.isfinite(r[k_]).all() for r in (r64, r32) for k_ in ("y", "dproj"))
    assert float(r64["dproj"].abs().max()) > 0
