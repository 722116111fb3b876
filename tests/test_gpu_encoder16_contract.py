"""GPU: the 16-bit fused encoder (eamrl_encoder_fused16) against its contract ("16-bit encoder"), called
directly with the weights of tests/encoder16_cases.py.

Exact cases: integer-grid data on which the accumulation order inside an MFMA cannot matter, so the kernel equals the
float64 emulation bit for bit in the embeddings, every cache slot and the graph context, and leaves every element of the
cache buffer outside its slots alone; the rounding-free ones also through the fp32 fused kernel.
Policy-scale cases: per node row, at most POLICY_FACTOR times the error that fp32 accumulation alone makes in the emulation
(the yardstick never sees the kernel).  test_host_encoder16_contract.py shows that these comparisons reject sixteen one-line
variants of the contract."""
import numpy as np
import pytest
import torch

import encoder16_cases as cases
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
E = cases.E
SENTINEL = -12345.0
_PACKED = ("Wqkv", "Wo", "W1", "W2")


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def _run(h, layers, cache, norm, eps, kind, pad=0):
    """The kernel (kind None: the fp32 fused kernel) on numpy inputs -> ({output: numpy}, the whole cache buffer with one
    guard instance behind the last, or None)."""
    from eam_rl4co_amd import ops

    dtype = DT[kind] if kind else None
    pack = (lambda W: ops.pack_linear_weight16(_dev(W), dtype)) if kind else (lambda W: ops.pack_linear_weight(_dev(W)))
    lay = [{n: (pack(v) if n in _PACKED else _dev(v)) for n, v in Ly.items()} for Ly in layers]
    B, M, _ = h.shape
    arg, big, gctx = None, None, None
    if cache is not None:
        nproj = cache["nproj"]
        big = torch.full((B + 1, M, (nproj + 1) * E + pad), SENTINEL, device=DEV)
        arg = (pack(cache["Wc"]), pack(cache["WoutT"]), big[:B], nproj)
        if cache.get("Wg") is not None:
            gctx = torch.full((B, E), SENTINEL, device=DEV)
            arg += (_dev(cache["Wg"]), gctx)
    code = ops.NORM_BATCH_EVAL if norm == "batch" else ops.NORM_INSTANCE
    if kind:
        out = ops.encoder_fused16(_dev(h), lay, 8, cases.FF, code, eps, dtype, cache=arg)
    else:
        out = ops.encoder_fused(_dev(h), lay, 8, cases.FF, code, eps, cache=arg)
    torch.cuda.synchronize()
    got = {"h": out.cpu().numpy()}
    if big is not None:
        big = big.cpu().numpy()
        for s, name in enumerate(cases.CACHE_SLOTS[nproj]):
            got[name] = big[:B, :, s * E:(s + 1) * E]
        if gctx is not None:
            got["gctx"] = gctx.cpu().numpy()
    return got, big


def _assert_bits(got, ref, what):
    """Bit equality with the emulation (+0 == -0: the sign of a zero carries no information here); on failure the first
    differing (instance, row, column)."""
    ref32 = np.asarray(ref, np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref), f"{what}: the reference is not fp32"
    assert got.shape == ref32.shape, f"{what}: shape {got.shape} vs {ref32.shape}"
    same = (got.view(np.uint32) == ref32.view(np.uint32)) | ((got == 0) & (ref32 == 0))
    if not same.all():
        first = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} elements differ, first at (instance, row, column) "
                             f"{first}: kernel {got[first]!r}, contract {ref32[first]!r}")


def _check_exact(case, kind, ref_kind):
    h, layers, cache = cases.exact_inputs(case)
    ref, _ = cases.exact_reference(case, ref_kind)
    got, big = _run(h, layers, cache, "batch", 0.0, kind, case.pad)
    assert set(got) == set(ref)
    for name in ref:
        _assert_bits(got[name], ref[name], f"{cases.exact_id(case)} {kind or 'fp32'} {name}")
    if big is not None:
        used = (case.nproj + 1) * E
        assert (big[:case.B, :, used:] == SENTINEL).all(), "columns past the last slot were written"
        assert (big[case.B] == SENTINEL).all(), "rows past the last instance were written"


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.EXACT_CASES, ids=cases.exact_id)
def test_fused16_exact_cases_equal_the_contract_bit_for_bit(case, kind):
    _check_exact(case, kind, kind)


@pytest.mark.parametrize("case", [c for c in cases.EXACT_CASES if c.rounding_free], ids=cases.exact_id)
def test_fused_fp32_equals_the_contract_on_rounding_free_cases(case):
    """No rounding point moves a value in these cases, so the contract's result is also the fp32 encoder's."""
    _check_exact(case, None, "bf16")


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.POLICY_CASES, ids=cases.policy_id)
def test_fused16_policy_scale_rows_follow_the_contract(case, kind):
    h, layers, cache, eps = cases.policy_inputs(case)
    got, _ = _run(h, layers, cache, case.norm, eps, kind)
    ratios = cases.policy_ratios(case, kind, got)
    factor = cases.policy_factor(case.stage, case.norm, kind)
    print(f"{cases.policy_id(case)} {kind}: " + " ".join(f"{n}={r.max():.2f}" for n, r in ratios.items()))
    for name, r in ratios.items():
        assert np.isfinite(got[name]).all(), name
        row = np.unravel_index(int(r.argmax()), r.shape)
        assert r.max() <= factor.get(name, cases.POLICY_FACTOR), \
            f"{name}: row {row} is {r.max():.2f} x the yardstick of ({case.stage}, {case.norm}, {kind})"
