"""The encoder self-attention forward at the small shapes the shared row-pair and plain code can get wrong and the other tests do
not reach, ops.mha_encoder against oracle.mha_encoder bit for bit: one node (k_mha_encoder_x2's pair with no second row), two
and three, a 16-row tile exactly and one over, 33; each through the default dispatch (k_mha_encoder_x2) and under debug key 3
(k_mha_encoder<16>); a qkv that starts 4 bytes off a 16-byte boundary (k_mha_encoder<16>); heads of 32 (k_mha_encoder<32>).
Every case asks eamrl_mha_encoder_variant which kernel it ran."""
import numpy as np
import pytest
import torch

from test_gpu_attention_large import _assert_bits_equal

pytestmark = pytest.mark.gpu

DEV = "cuda"
X2, PLAIN16, PLAIN32 = 1, 4, 5          # EAMRL_MHA_* (include/eamrl.h; tests/test_host_mha_dispatch.py checks the values)


def _run(qkv, H, key3=False):
    """-> (y, the EAMRL_MHA_* id of the kernel that computed it)."""
    from eam_rl4co_amd import _lib, ops

    lib = _lib.load()
    lib.eamrl_debug_set(3, int(key3))
    try:
        y = ops.mha_encoder(qkv, H)
        torch.cuda.synchronize()
        B, N, E3 = qkv.shape
        return y, lib.eamrl_mha_encoder_variant(qkv.data_ptr(), y.data_ptr(), B, N, E3 // 3, H)
    finally:
        lib.eamrl_debug_set(3, 0)


@pytest.mark.parametrize("N", [1, 2, 3, 16, 17, 33])
def test_small_graphs_are_the_oracle_bit_for_bit(oracle, N):
    qkv = np.random.default_rng(900 + N).standard_normal((2, N, 384)).astype(np.float32) * 1.5
    ref = oracle.mha_encoder(qkv, 8)
    assert np.isfinite(ref).all()
    for key3, want in ((False, X2), (True, PLAIN16)):
        y, variant = _run(torch.from_numpy(qkv).to(DEV), 8, key3)
        assert variant == want
        _assert_bits_equal(y, ref, f"N = {N}, variant {variant}")


def test_misaligned_qkv_takes_the_plain_kernel(oracle):
    B, N = 2, 17
    qkv = np.random.default_rng(917).standard_normal((B, N, 384)).astype(np.float32) * 1.5
    buf = torch.zeros(B * N * 384 + 4, device=DEV)
    view = buf[1:1 + B * N * 384].view(B, N, 384)
    view.copy_(torch.from_numpy(qkv))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    y, variant = _run(view, 8)
    assert variant == PLAIN16
    _assert_bits_equal(y, oracle.mha_encoder(qkv, 8), "qkv 4 bytes off")


def test_heads_of_32(oracle):
    qkv = np.random.default_rng(932).standard_normal((1, 5, 768)).astype(np.float32) * 1.5
    y, variant = _run(torch.from_numpy(qkv).to(DEV), 8)
    assert variant == PLAIN32
    _assert_bits_equal(y, oracle.mha_encoder(qkv, 8), "D = 32")
