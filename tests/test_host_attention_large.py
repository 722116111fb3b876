"""The large-graph encoder attention tests' own ground, checked without a GPU and without the package: the case list
(tests/attn_large_cases.py) with every named size on the kernel edge it is named for, the float64 restatement
(tests/train_ref.py: attention_backward) against torch's float64 autograd through scaled_dot_product_attention, the soundness of
every case (bounds that the float32 restatement meets, data kinds that are what they claim), and four planted errors per backward
case that the bound must reject.
"""
import pytest
import torch
import torch.nn.functional as F

import attn_large_cases as ac


def test_case_list_is_the_one_promised():
    cs = ac._build()
    assert len(cs) == len(ac.NAMES) == len(set(ac.NAMES))
    n = set(ac.NAMES)
    normal = (113, 127, 128, 129, 256, 257, 272, 273, 384, 385, 512, 513, 640, 641, 768, 769, 896, 897, 1023, 1024)
    assert {f"normal_N{N}" for N in normal} | {f"peaked_N{N}" for N in (129, 641, 1024)} | {"twin_N257", "zero_rows_N385"} <= n
    assert {"dominant_N113_k112", "dominant_N273_k272", "dominant_N641_k640", "dominant_N1024_k1023", "dominant_N1024_k0",
            "dominant_N897_k115"} | {f"fwd_normal_N{N}" for N in (1185, 1200, 1201, 1281)} <= n
    assert len(n) == len(normal) + 3 + 2 + 6 + 4
    for c in ac.CASES.values():
        assert (c["B"], c["backward"]) == ((1, False) if c["name"].startswith("fwd_") else (2, True))
        assert c["kind"] in ac.KINDS and (c["dom"] is not None) == (c["kind"] == "dominant")
        assert 113 <= c["N"] <= 1024 or not c["backward"]
    assert {c["kind"] for c in ac.CASES.values()} == set(ac.KINDS)
    assert set(ac.ORACLE_SIZES) == {128, 129, 144, 145, 160, 161, 176, 177, 192, 193, 511, 512, 513, 1023, 1024, 1185, 1200, 1201,
                                    1281}
    assert ac.MARGIN == 4.0 and all(v >= 1.0 for v in ac.RATIO.values())


def test_cases_sit_on_the_edges_they_are_named_for():
    # k_mha_encoder_bwd_mfma<U>: U = ceil(ceil(N / 16) / 8); both sides of every step, so that all eight instantiations run
    want_u = {113: 1, 127: 1, 128: 1, 129: 2, 256: 2, 257: 3, 272: 3, 273: 3, 384: 3, 385: 4, 512: 4, 513: 5, 640: 5, 641: 6, 768: 6,
              769: 7, 896: 7, 897: 8, 1023: 8, 1024: 8}
    assert {N: ac.bwd_tiles_per_wave(N) for N in want_u} == want_u
    assert set(want_u) == {c["N"] for c in ac.CASES.values() if c["backward"]}
    assert {ac.bwd_tiles_per_wave(c["N"]) for c in ac.CASES.values() if c["kind"] == "normal" and c["backward"]} == set(range(1, 9))
    for lo, hi in zip(ac.BWD_U_STEPS[::2], ac.BWD_U_STEPS[1::2]):
        assert hi == lo + 1 and ac.bwd_tiles_per_wave(hi) == ac.bwd_tiles_per_wave(lo) + 1
    assert ac.bwd_tiles_per_wave(1025) == 9          # (no instantiation: the launcher's default branch)
    # 113: the last key tile holds one key; 1023: fifteen
    assert (ac.key_tiles(113), 113 - 16 * 7) == (8, 1) and (ac.key_tiles(1023), 1023 - 16 * 63) == (64, 15)
    # the backward's dynamic LDS: both sides of the 64 KiB attribute, and the largest graph inside the 160 KiB of a workgroup
    assert (ac.bwd_lds_bytes(272), ac.bwd_lds_bytes(273)) == (64512, 66560) and 64512 <= 64 * 1024 < 66560
    assert ac.bwd_lds_bytes(1024) == 160768 <= 160 * 1024
    # twin: nodes 0 and N - 2 = 255 in the tiles of different waves (0 and 15 -> waves 0 and 7)
    assert (0 // 16) % 8 != (255 // 16) % 8
    # dominant: the last key alone in its tile (113, 273, 641), last in a full tile (1024), key 115 the first tile of wave 7
    assert [N - 1 - (N - 1) // 16 * 16 for N in (113, 273, 641, 1024)] == [0, 0, 0, 15]
    assert (115 // 16, 115 // 16 % 8, ac.bwd_tiles_per_wave(897)) == (7, 7, 8)
    for N, dom in ac.BWD_DOMINANT:      # seven of the eight waves do not hold the dominant key
        assert sum(any(kt * 16 <= dom < kt * 16 + 16 for kt in range(w, ac.key_tiles(N), 8)) for w in range(8)) == 1
    # k_mha_encoder_mfma: (NT, NT % 4, bytes of LDS) at the oracle's sizes; the four-tile score groups clamp 4 - NT % 4 tiles
    want_f = {128: (8, 0, 16384), 129: (9, 1, 18432), 144: (9, 1, 18432), 145: (10, 2, 20480), 160: (10, 2, 20480),
              161: (11, 3, 22528), 176: (11, 3, 22528), 177: (12, 0, 24576), 192: (12, 0, 24576), 193: (13, 1, 26624),
              511: (32, 0, 65536), 512: (32, 0, 65536), 513: (33, 1, 67584), 1023: (64, 0, 131072), 1024: (64, 0, 131072),
              1185: (75, 3, 153600), 1200: (75, 3, 153600), 1201: (76, 0, 155648), 1281: (81, 1, 165888)}
    assert set(want_f) == set(ac.ORACLE_SIZES)
    for N, w in want_f.items():
        assert (ac.key_tiles(N), ac.key_tiles(N) % 4, ac.fwd_lds_bytes(N)) == w, N
    assert {ac.key_tiles(N) % 4 for N in ac.ORACLE_SIZES if N <= 193} == {0, 1, 2, 3}
    assert 65536 <= 64 * 1024 < 67584 and 153600 == 150 * 1024           # the raised attribute from 513, the limit at 1200
    assert 1185 - 16 * 74 == 1                                            # NT = 75 with one key in the last tile
    assert [ac.fwd_kernel(N) for N in (128, 512, 513, 1200, 1201, 1281)] == ["mfma"] * 4 + ["tiled"] * 2
    assert all(ac.fwd_kernel(N, key15=True) == "tiled" for N in ac.ORACLE_SIZES)
    assert {ac.fwd_kernel(c["N"]) for c in ac.CASES.values() if not c["backward"]} == {"mfma", "tiled"}
    # k_mha_encoder_tiled: tiles of 128 keys; 1281 = 10 x 128 + 1
    assert {128, 129, 512, 513, 1024} <= set(ac.ORACLE_SIZES) and divmod(1281, 128) == (10, 1)


def _autograd(op):
    """torch's own float64 autograd through scaled_dot_product_attention -> the outputs under the restatement's names."""
    qkv = op["qkv"].double().requires_grad_()
    B, N, _ = qkv.shape
    q = qkv.view(B, N, 3, ac.H, ac.D).permute(2, 0, 3, 1, 4)
    y = F.scaled_dot_product_attention(q[0], q[1], q[2]).permute(0, 2, 1, 3).reshape(B, N, ac.E)
    y.backward(op["dout"].double())
    return ac.split(y.detach(), qkv.grad)


@pytest.mark.parametrize("name", ac.NAMES)
def test_float64_restatement_equals_torch_autograd(name):
    op, r64, _ = ac.reference(name)
    want = _autograd(op)
    for k in ac.OUTPUTS:
        scale = max(float(want[k].abs().max()), r64["_scale"][k])
        assert float((r64[k] - want[k]).abs().max()) <= 1e-12 * scale, k


@pytest.mark.parametrize("name", ac.NAMES)
def test_case_is_sound(name):
    c = ac.CASES[name]
    op, r64, r32 = ac.reference(name)
    N, kind = c["N"], c["kind"]
    assert op["qkv"].shape == (c["B"], N, 3 * ac.E) and op["dout"].shape == (c["B"], N, ac.E)
    for k in ac.OUTPUTS:
        assert torch.isfinite(r64[k]).all() and torch.isfinite(r32[k]).all(), k
        assert ac.bound(c, k, r64, r32)[1] > 0 and r64["_scale"][k] > 0, k
    assert ac.misses(c, r32, r64, r32, ac.OUTPUTS) == []          # the float32 restatement meets its own bound
    assert ac.outputs(c) == (list(ac.OUTPUTS) if c["backward"] else ["y"])
    p = ac.weights(op)
    if kind == "dominant":              # the one key holds 0.98 .. 0.9999 of every row, and the gradients are not empty
        w = p[..., c["dom"]]
        assert 0.98 <= float(w.min()) and float(w.max()) <= 0.9999, (float(w.min()), float(w.max()))
        assert float(r64["dq"].norm()) >= 0.01 and float(r64["dk"].norm()) >= 0.01
    if kind == "peaked":
        assert float(p.max()) > 0.999
    if kind == "twin":
        assert torch.equal(op["qkv"][:, 0], op["qkv"][:, N - 2]) and not torch.equal(op["qkv"][:, 0], op["qkv"][:, 1])
    if kind == "zero_rows":
        rows = list(ac.ZERO_ROWS)
        assert float(op["dout"][:, rows].abs().max()) == 0.0 and float(r64["dq"][:, rows].abs().max()) == 0.0
        assert float(op["dout"].abs().sum(-1).min(1).values.max()) == 0.0 and int((op["dout"].abs().sum(-1) == 0).sum()) == 3 * c["B"]


@pytest.mark.parametrize("name", ac.BACKWARD)
def test_bound_rejects_the_planted_errors(name):
    """Copies of the float64 outputs with the last key, the last key tile or one wave's key tiles not attended to, and one with the
    last query tile left out of dk and dv: each lies beyond the case's bound in an output the error reaches."""
    c = ac.CASES[name]
    op, r64, r32 = ac.reference(name)
    for which in ac.PLANTS:
        if (name, which) == ("zero_rows_N385", "last_query_tile_skipped"):      # that tile is the one row N - 1, and its dout is zero
            assert ac.planted(name, which) is None and c["N"] % 16 == 1 and -1 in ac.ZERO_ROWS
            continue
        got, reached = ac.planted(name, which)
        bad = ac.misses(c, got, r64, r32, reached)
        assert bad, (name, which)
        if which == "last_query_tile_skipped":      # y and dq untouched by construction
            assert torch.equal(got["y"], r64["y"]) and torch.equal(got["dq"], r64["dq"])
            assert {b[0] for b in bad} == {"dk", "dv"}
