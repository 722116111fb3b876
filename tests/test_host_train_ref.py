"""The training-graph kernel tests' own ground, checked without a GPU and without the package: the restatements
(tests/train_ref.py) against torch's float64 autograd of the operations they restate, the soundness of every case
(tests/train_cases.py: shapes on the branch edges they are named for, bounds that the float32 restatement meets), and three
planted errors per case that the bound must reject.
"""
import pytest
import torch
import torch.nn.functional as F

import train_cases as tc
import train_ref as tr


def test_case_list_is_the_one_promised():
    cs = tc._build()
    assert len(cs) == len(tc.NAMES) == len(set(tc.NAMES))
    n = set(tc.NAMES)
    assert {f"lin_r{r}_128x128" for r in (1, 15, 16, 17, 63, 64, 193, 769, 1025, 32769)} | {"lin_r65_128x128_noaux"} <= n
    assert {f"lin_r{r}_{s}" for r in (65, 777) for s in ("384x128", "128x512", "512x512")} | {"lin_r2049_512x512_noaux"} <= n
    assert {f"sm_r257_K{K}_o128" for K in range(1, 9)} | {f"sm_r{r}_K2_o128" for r in (1, 255, 256, 2000)} <= n
    assert {c["out"] for c in tc.CASES.values() if c["fam"] == "small"} == {64, 100, 128, 300}
    assert {f"in_B3_N{N}_E128" for N in (1, 2, 3, 4, 5, 126, 127, 190, 191, 300)} | {"in_B600_N20_E128", "in_B1_N20_E128"} <= n
    assert {f"in_B3_N20_E{E}" for E in (6, 64, 130, 300)} | {"in_B3_N20_E200_noaux", "in_B2_N188_E130"} <= n
    assert {f"bn_r{r}_E128" for r in (1, 2, 127, 128, 5000, 32769)} | {"bn_r129_E128_noaux"} <= n
    assert {c["E"] for c in tc.CASES.values() if c["fam"] == "bn"} == {4, 64, 128, 200, 1028, 2048}
    assert {f"at_N{N}_a1.5" for N in (1, 2, 15, 16, 17, 63, 64, 65, 111, 112)} | {"at_N112_a6", "at_N33_a1.5_tie"} <= n
    for fam, kinds in (("linear", {"normal", "offset"}), ("small", {"normal", "offset"}), ("attn", {"normal"}),
                       ("instnorm", {"normal", "offset", "const", "tiny"}), ("bn", {"normal", "offset", "const", "tiny"})):
        assert {c["kind"] for c in tc.CASES.values() if c["fam"] == fam} == kinds
        assert any(c["no_aux"] for c in tc.CASES.values() if c["fam"] == fam) or fam == "attn"


def test_cases_sit_on_the_branch_edges_they_are_named_for():
    # k_linear_wgrad: declared chunk counts are the launch rule's, and the rows of the last chunks are what the comments say
    for c in tc.CASES.values():
        if c["fam"] == "linear":
            assert tc.linear_chunks(c["rows"], c["out"], c["inp"])[0] == c["nch"], c["name"]

    def last(rows, o, i):          # (rows per chunk, index of the last non-empty chunk, its rows)
        nch, rpc = tc.linear_chunks(rows, o, i)
        k = (rows - 1) // rpc
        return rpc, k, rows - k * rpc

    assert last(65, 128, 128) == (48, 1, 17) and last(193, 128, 128) == (64, 3, 1) and last(769, 128, 128) == (64, 12, 1)
    assert last(1025, 128, 128) == (64, 16, 1) and last(2049, 512, 512) == (80, 25, 49) and last(32769, 128, 128) == (80, 409, 49)
    # k_instnorm_train_fwd: bytes of dynamic shared memory and the regime
    want = {(126, 128): (65536, "lds"), (127, 128): (66048, "lds_raised"), (190, 128): (98304, "lds_raised"),
            (191, 128): (98816, "global"), (300, 128): (154624, "global"), (187, 130): (98280, "lds_raised"),
            (188, 130): (98800, "global"), (20, 300): (26400, "lds")}
    for (N, E), w in want.items():
        assert tc.instnorm_lds(N, E) == w
        assert any(c["fam"] == "instnorm" and (c["N"], c["E"]) == (N, E) for c in tc.CASES.values())
    # k_bn_bwd_dx: 4096 workgroups of 256 threads, one float4 each per trip
    assert 32769 * 128 // 4 > 4096 * 256 >= 32768 * 128 // 4


def _autograd(c, op):
    """torch's own float64 autograd of the operation -> dict of the outputs it defines."""
    fam = c["fam"]
    d = {k: v.double() for k, v in op.items()}
    if fam in ("linear", "small"):
        W = torch.zeros(c["out"], d["x"].shape[1], dtype=torch.float64, requires_grad=True)
        b = torch.zeros(c["out"], dtype=torch.float64, requires_grad=True)
        F.linear(d["x"], W, b).backward(d["dy"])
        return dict(dW=W.grad, db=b.grad)
    if fam in ("instnorm", "bn"):
        x, g, b = d["x"].requires_grad_(), d["gamma"].requires_grad_(), d["beta"].requires_grad_()
        n = c["N"] if fam == "instnorm" else c["rows"]
        if n == 1:          # (torch refuses one value per channel in training mode: the definition, written out)
            dim = 1 if fam == "instnorm" else 0
            m = x.mean(dim, keepdim=True)
            y = (x - m) / torch.sqrt(((x - m) ** 2).mean(dim, keepdim=True) + tc.EPS) * g + b
        elif fam == "instnorm":
            y = F.instance_norm(x.permute(0, 2, 1), weight=g, bias=b, eps=tc.EPS).permute(0, 2, 1)
        else:
            y = F.batch_norm(x, None, None, g, b, True, 0.0, tc.EPS)
        y.backward(d["dy"])
        out = dict(dx=x.grad, dgamma=g.grad, dbeta=b.grad)
        if fam == "instnorm":
            out["y"] = y.detach()
        return out
    qkv = d["qkv"].requires_grad_()
    B, N, _ = qkv.shape
    q = qkv.view(B, N, 3, tc.H, tc.E_ATT // tc.H).permute(2, 0, 3, 1, 4)
    y = F.scaled_dot_product_attention(q[0], q[1], q[2]).permute(0, 2, 1, 3).reshape(B, N, tc.E_ATT)
    y.backward(d["dout"])
    return dict(y=y.detach(), dqkv=qkv.grad)


@pytest.mark.parametrize("name", tc.NAMES)
def test_float64_restatement_equals_torch_autograd(name):
    c = tc.CASES[name]
    op, r64, _ = tc.reference(name)
    want = _autograd(c, {k: v for k, v in op.items() if k not in ("mean", "var")})
    assert set(tc.outputs(c)) - {"mean", "rstd"} <= set(want)
    # The norms' outputs go through x - mean, whose float64 rounding (in torch's kernels as in the restatement) is 2^-53 |x|, and
    # which rstd then multiplies: per channel the scale of such an output is its magnitude times max |x| rstd where that exceeds 1
    # (1000 on the offset data, 316,000 in the constant channel of 1000; about 3 on the normal data).
    cond = 1.0
    if c["fam"] in ("instnorm", "bn"):
        x = op["x"].double()
        rstd = r64["rstd"].amax(0) if c["fam"] == "instnorm" else 1 / torch.sqrt(r64["var"] + tc.EPS)
        cond = (x.abs().reshape(-1, c["E"]).amax(0) * rstd).clamp_min(1.0)          # [E]
    for k, w in want.items():
        scale = max(float(w.abs().max()), r64["_scale"][k])
        assert bool(((r64[k] - w).abs() <= 1e-12 * scale * cond).all()), k
    if c["fam"] == "instnorm":      # the kept statistics, from their definitions
        x = op["x"].double()
        assert torch.equal(r64["mean"], x.mean(1))
        var = x.var(1, unbiased=False) if c["N"] > 1 else torch.zeros_like(r64["mean"])
        assert float((r64["rstd"] - 1 / torch.sqrt(var + tc.EPS)).abs().max()) <= 1e-12 * float(r64["rstd"].max())
    if c["fam"] == "bn":
        x = op["x"].double()
        assert torch.equal(r64["mean"], x.mean(0))
        assert float((r64["var"] - x.var(0, unbiased=False)).abs().max()) <= 1e-12 * max(float(r64["var"].max()), 1e-30)


@pytest.mark.parametrize("name", tc.NAMES)
def test_case_is_sound(name):
    c = tc.CASES[name]
    op, r64, r32 = tc.reference(name)
    for k in tc.outputs(c):
        assert k in r64 and k in r32 and torch.isfinite(r64[k]).all() and torch.isfinite(r32[k]).all(), k
        # a bound of zero asks for the exact result: only where the result is exactly zero
        kind, bd = tc.bound(c, k, r64, r32)
        assert bd > 0 or float(r64[k].abs().max()) == 0.0, k
    assert tc.misses(c, r32, r64, r32) == []          # the float32 restatement meets its own floor-aware bound
    fam, kind = c["fam"], c["kind"]
    n = c.get("N") if fam == "instnorm" else c.get("rows")
    if fam in ("instnorm", "bn") and n == 1:          # the exactly-zero outputs
        assert all(float(r64[k].abs().max()) == 0.0 for k in ("dx", "dgamma"))
        assert float(r64["dbeta"].abs().max()) > 0
    if kind == "const":                               # zero variance exactly, y == beta, mean == the constant
        ch = list(tc.const_channels(c["E"]))
        var = r64["var"][ch] if fam == "bn" else 1 / r64["rstd"][:, ch] ** 2 - tc.EPS
        assert float(var.abs().max()) <= 1e-18
        assert torch.equal(r64["mean"][..., ch], torch.tensor(tc.CONST_VALUES, dtype=torch.float64).expand_as(r64["mean"][..., ch]))
        assert float(r64["dgamma"][ch].abs().max()) == 0.0
        if fam == "instnorm":
            assert torch.equal(r64["y"][..., ch], op["beta"].double()[ch].expand_as(r64["y"][..., ch]))
            # ... and a float32 sum of the constants in node order is exact: the property the constants were chosen for
            s = torch.zeros(len(ch))
            for _ in range(c["N"]):
                s = s + torch.tensor(tc.CONST_VALUES)
            assert torch.equal(s / c["N"], torch.tensor(tc.CONST_VALUES))
    if kind == "offset" and fam in ("linear", "small"):       # the sum nearly cancels: far below the sum of |terms|
        assert float(r64["db"].abs().max()) <= 0.1 * r64["_scale"]["db"]
        assert float(r64["dW"].abs().max()) <= 0.1 * r64["_scale"]["dW"]
    if kind == "tiny":                                # the variance vanishes beside eps
        rstd = r64["rstd"] if fam == "instnorm" else 1 / torch.sqrt(r64["var"] + tc.EPS)
        assert float((rstd * tc.EPS ** 0.5 - 1).abs().max()) <= 1e-12
    if fam == "attn":
        p_max = float(torch.softmax((op["qkv"].double()[..., :128].view(c["B"], c["N"], 8, 16).transpose(1, 2) @
                                     op["qkv"].double()[..., 128:256].view(c["B"], c["N"], 8, 16).transpose(1, 2).transpose(-1, -2)) / 4,
                                    -1).max())
        if c["amp"] == 6:
            assert p_max > 0.999
        if c.get("tie"):
            assert torch.equal(op["qkv"][:, 0], op["qkv"][:, c["N"] - 2])


@pytest.mark.parametrize("name", tc.NAMES)
def test_bound_rejects_the_planted_errors(name):
    """A copy of the float64 outputs with one row of the contraction dropped, one with the last chunk (slab, key tile, row group)
    left out, and on `offset` data one computed with a one-pass variance: each lies beyond the case's bound."""
    c = tc.CASES[name]
    op, r64, r32 = tc.reference(name)
    seen = []
    for which in tc.PLANTS:
        got = tc.planted(name, which)
        if got is None:
            continue
        seen.append(which)
        assert tc.misses(c, got, r64, r32), (name, which)
    fam = c["fam"]
    n = c["N"] if fam in ("instnorm", "attn") else c["rows"]
    # where a plant does not apply: a contraction of one term (the norms, one key), fewer nodes than four row groups, one key tile
    want = ["row_dropped"] if n >= 2 or fam in ("linear", "small") else []
    want += ["last_chunk_dropped"] if fam in ("linear", "small") or (fam == "bn" and n >= 2) or (fam == "instnorm" and n >= 4) or \
        (fam == "attn" and n > 16) else []
    want += ["one_pass_variance"] if c["kind"] == "offset" and fam in ("instnorm", "bn") else []
    assert seen == want
