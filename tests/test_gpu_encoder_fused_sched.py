"""GPU: the software-pipelined GEMM passes of the fused fp32 encoder (k-group u + 1's fragments in flight under the MFMAs of
group u, first fragments of a pass requested ahead of the preceding barrier) at the shapes where a mis-pipelined pass goes
wrong -- a fragment of group u + 1 consumed in group u, a row-tile count off by one: every kernel variant (2, 4, 7 row tiles),
both row-tile counts of a wave half, full and partial last tiles.  Bit for bit against the layer-by-layer kernels of
encoder.hip, like test_gpu_encoder_fused.py."""
import pytest
import torch

from test_gpu_parity import DEV, assert_bits_equal, make_policy

pytestmark = pytest.mark.gpu

B = 3
NODES = [1, 16, 17, 32, 33, 64, 65, 96, 97, 100, 112]
CONFIGS = ["am_tsp", "pomo_tsp"]          # 3 layers, batch norm (eval) | 6 layers, instance norm


@pytest.mark.parametrize("M", NODES)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_pipelined_passes_are_bit_identical(monkeypatch, cfg, M):
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import ops

    env = ea.get_env("tsp", generator_params=dict(num_loc=M), seed=M + 5)
    torch.manual_seed(M * 13 + B)
    td = env.reset(batch_size=[B]).to(DEV)
    pol = make_policy(cfg)
    assert td["locs"].shape[1] == M and ops.encoder_fused_supported(M, 128, 8, 512, len(pol.encoder.net.layers))
    with torch.no_grad():
        # reference: one launch per Linear / attention / norm, the cache by GEMM launches
        monkeypatch.setenv("EAMRL_FUSED_ENCODER", "0")
        monkeypatch.setenv("EAMRL_FUSED_CACHE", "0")
        h_ref, init_ref = pol.encoder(td)
        cache_ref = pol.decoder._precompute_cache(h_ref).buf.clone()
        monkeypatch.delenv("EAMRL_FUSED_ENCODER")
        monkeypatch.delenv("EAMRL_FUSED_CACHE")
        # embeddings given, no cache
        h, init = pol.encoder(td)
        assert_bits_equal(init, init_ref, "init embeddings")
        assert_bits_equal(h, h_ref, f"h_in, no cache (M={M})")
        # in-kernel init embedding, cache
        spec_i = pol.decoder._fused_cache_spec(B, M, DEV)
        h, init = pol.encoder(td, cache_spec=spec_i)
        assert spec_i["filled"]
        assert_bits_equal(init, init_ref, "in-kernel init embeddings")
        assert_bits_equal(h, h_ref, f"in-kernel init, cache (M={M})")
        assert_bits_equal(spec_i["buf"], cache_ref, f"cache, in-kernel init (M={M})")
        # embeddings given, cache
        monkeypatch.setenv("EAMRL_FUSED_INIT", "0")
        spec_h = pol.decoder._fused_cache_spec(B, M, DEV)
        h, _ = pol.encoder(td, cache_spec=spec_h)
        assert spec_h["filled"]
        assert_bits_equal(h, h_ref, f"h_in, cache (M={M})")
        assert_bits_equal(spec_h["buf"], cache_ref, f"cache, h_in (M={M})")
        if spec_h.get("gctx") is not None:
            assert_bits_equal(spec_i["gctx"], spec_h["gctx"], "graph context")
