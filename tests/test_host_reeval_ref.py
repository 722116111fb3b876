"""The re-evaluation tests' own ground, checked without a GPU: the restatement of the operator (tests/reeval_ref.py) against the
logits recorded from the reference's PointerAttention.forward, the bit-packing helpers, the soundness of every synthetic case
(tests/reeval_cases.py), and eight one-line mutants of the restatement, each of which the named case must see beyond its bound.

Which case catches which mutant (the pair is the test's parameter; any output beyond the case's bound counts):
  instance r // S for r % B ............................ ops_pb
  tstart ignored ....................................... ops_pb
  idxB ignored ......................................... ops_pb
  1 / temp dropped from the gradient only .............. temp0.5_M20
  1 - tanh^2 dropped ................................... peaked_M20
  mask on the logits but not on the glimpse ............ ops_pb
  entropy as lse - sum p z with z unclipped ............ peaked_M20
  rem of step t - 1 used at step t ..................... ops_dyn_M20
"""
import math

import numpy as np
import pytest
import torch

import reeval_cases as rc
import reeval_ref as rr
from _util import golden


@pytest.mark.parametrize("tag", ["single", "multi", "wide"])
def test_restatement_reproduces_the_recorded_reference_logits(tag):
    """glimpse + logits of the restatement in float64 against the reference module's recorded output: the differences are the
    float32 rounding of the recording (1.5e-7 at most)."""
    import goldweights

    fx = golden("pointer_attention")
    kvl = torch.from_numpy(fx[f"{tag}_kvl"]).double()
    K, V, LK = (kvl[..., i * rr.E:(i + 1) * rr.E] for i in range(3))
    Wout = torch.from_numpy(goldweights.tensor_for("decoder.pointer.project_out.weight", (rr.E, rr.E))).double()
    Lp = LK @ Wout                                    # logit_key . project_out(heads) = (logit_key Wout) . heads
    q = torch.from_numpy(fx[f"{tag}_q"]).double()
    mask = torch.from_numpy(fx[f"{tag}_mask"])
    if mask.dim() == 2:
        mask = mask[:, None, :]
    _, u, _ = rr.glimpse_logits(q, K, V, Lp, mask.expand(q.shape[0], q.shape[1], -1))
    want = fx[f"{tag}_logits"].reshape(u.shape)
    np.testing.assert_allclose(u.numpy(), want, rtol=0, atol=1e-6)


def test_bit_packing_helpers_round_trip():
    rng = np.random.default_rng(3)
    for M in (1, 31, 32, 33, 64, 96, 112):
        mask = rng.random((3, 2, M)) < 0.5
        for n in (31, 32, 63, 64, 95, 96, 111):
            if n < M:
                mask[0, 0, n], mask[1, 0, n] = True, False
        words = rr.pack_mask_bits(mask).numpy().view(np.uint32)
        assert words.shape == (3, 2, 4)
        back = (words[..., None] >> np.arange(32, dtype=np.uint32)) & 1
        back = back.reshape(3, 2, 128)
        assert np.array_equal(back[..., :M].astype(bool), mask) and not back[..., M:].any()
    for M in (114, 224, 225, 500):
        nkc = -(-M // 112)
        mask = rng.random((2, 3, M)) < 0.5
        for n in (31, 32, 63, 64, 95, 96, 111, 112, 113):
            mask[0, 0, n], mask[1, 0, n] = True, False
        words = rr.pack_mask_bits_chunked(mask).numpy().view(np.uint32)
        assert words.shape == (2, 3, nkc, 4)
        back = ((words[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(2, 3, nkc, 128)
        assert not back[..., 112:].any()                       # a chunk holds 112 nodes
        back = back[..., :112].reshape(2, 3, nkc * 112)
        assert np.array_equal(back[..., :M].astype(bool), mask) and not back[..., M:].any()
        rem = torch.from_numpy(rng.random((2, 3, M)).astype(np.float32))
        rows = rr.rem_rows(rem)
        assert rows.shape == (2, 3, nkc, 128) and not rows[..., 112:].any()
        flat = rows[..., :112].reshape(2, 3, nkc * 112)
        assert torch.equal(flat[..., :M], rem) and not flat[..., M:].any()
    rem = torch.from_numpy(rng.random((2, 3, 20)).astype(np.float32))
    rows = rr.rem_rows(rem)
    assert rows.shape == (2, 3, 128) and torch.equal(rows[..., :20], rem) and not rows[..., 20:].any()


def test_case_list_is_the_one_promised():
    names = set(rc.NAMES)
    assert {f"edge_M{M}" for M in (1, 2, 15, 16, 17, 32, 33, 64, 65, 111, 112, 113, 224, 225)} <= names
    for M in (20, 65, 130):
        assert {f"{k}_M{M}" for k in ("peaked", "clip0", "temp0.5", "temp2", "forced", "tie", "policy")} <= names
    for name in ("rows_B512_S3_M8_T6", "rows_B100_S13_M33_T7", "rows_B64_S9_M20_T19", "rows_B100_S13_M113_T5"):
        c = rc.CASES[name]
        nchunk = max(1, min(c["S"], -(-512 // c["B"])))
        assert c["S"] / nchunk > 1 and c["T"] % 16 and c["tstart"] == 1        # more than one row in a workgroup
    assert [max(1, min(rc.CASES[n]["S"], -(-512 // rc.CASES[n]["B"]))) for n in rc.NAMES[:4]] == [1, 6, 8, 6]


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_is_sound(name):
    c = rc.CASES[name]
    op, glogp, r64, r32 = rc.reference(name)
    mask, actions = op["mask"], op["actions"]
    R, T = actions.shape
    act = r64["active"]
    assert mask.any(-1).all()                                               # no empty mask (the reference asserts on that)
    assert mask.gather(2, actions[..., None]).all()                         # every action feasible
    for r in (r64, r32):
        for k in rc.outputs(c) + ["heads", "u"]:
            assert torch.isfinite(r[k]).all(), k
    assert (r64["logp"][~act] == 0).all() and (r64["entropy"][~act] == 0).all() and (r64["logp"][act] <= 0).all()
    inst = torch.arange(R) % c["B"]
    if c["backward"]:
        for b in range(c["B"]):
            if rc.dead_node(c, b) >= 0:       # a node no query can see: zero gradient rows
                assert not mask[inst == b][:, :, rc.dead_node(c, b)].any()
                for k in ("dK", "dV", "dLp"):
                    assert (r64[k][b, rc.dead_node(c, b)] == 0).all()
        if rc.unindexed_node(c) >= 0:
            assert (r64["dPa"][:, rc.unindexed_node(c)] == 0).all() and (not c["pb"] or (r64["dPb"][:, rc.unindexed_node(c)] == 0).all())
            assert float(r64["dPa"].abs().max()) > 0
        for k in rc.exact_zero(c):
            assert float(r64[k].abs().max()) == 0.0
    # the property the case is named for
    u, attn = r64["u"][act], r64["attn"][act]
    if c["scale"] == "peaked":
        assert float(attn.max()) > 0.99 and float(u.abs().max()) > 3.0
        assert float((torch.tanh(u) ** 2).max()) > 0.99          # saturated clipping somewhere
    if c["scale"] == "policy":
        assert float(u.abs().max()) <= 0.6
    if c["forced"]:
        f = torch.arange(T) % rc.FORCED_EVERY[0] == rc.FORCED_EVERY[1]
        assert f[c["tstart"]:].any() and (mask[:, f].sum(-1) == 1).all()
        assert (r64["logp"][:, f] == 0).all() and (r64["entropy"][:, f] == 0).all()
        g0 = glogp.clone()
        g0[:, ~f] = 0                                   # the forced steps alone: exactly zero gradient
        alone = rr.reeval_with_grads(op, g0)
        assert all(float(alone[k].abs().max()) == 0.0 for k in rc.outputs(c) if k in rr.GRADS)
    if c["tie"]:
        f = torch.arange(T) % rc.TIE_EVERY[0] == rc.TIE_EVERY[1]
        n1, n2 = rc.tie_nodes(c)
        assert (mask[:, f].sum(-1) == 2).all() and mask[:, f][:, :, [n1, n2]].all()
        fa = f[None, :] & act
        np.testing.assert_allclose(r64["logp"][fa].numpy(), -math.log(2.0), rtol=0, atol=1e-15)
        np.testing.assert_allclose(r64["entropy"][fa].numpy(), math.log(2.0), rtol=0, atol=1e-15)
        for k in ("dK", "dV"):
            assert float(r64[k][:, n1].abs().max()) > 0
            np.testing.assert_allclose(r64[k][:, n1].numpy(), r64[k][:, n2].numpy(), rtol=1e-12, atol=1e-15)
    if c["mask"] == "edges":
        e = [n for n in rc.EDGE_NODES if n < c["M"]]
        for b in range(c["B"]):
            for n in e:
                if n != rc.dead_node(c, b):             # both states of every node next to a tile / word boundary
                    col = mask[inst == b][:, c["tstart"]:, n]
                    assert c["T"] - c["tstart"] < 2 or (col.any() and not col.all()), n
        if c["M"] > rr.KEY_CHUNK:
            last = rr.KEY_CHUNK * ((c["M"] - 1) // rr.KEY_CHUNK)
            assert not mask[:, 2, :last].any() and not mask[:, 3, rr.KEY_CHUNK:].any()
    if c["neg_idx"]:
        frac = float((op["idxA"] < 0).float().mean())
        assert 0.2 < frac < 0.45 and (op["idxB"] < 0).any()
    if c["idx_all"] is not None:
        assert (op["idxA"] == c["idx_all"]).all() and (not c["pb"] or (op["idxB"] == -1).all())
        nchunk = max(1, min(c["S"], -(-512 // c["B"])))
        if name == "gather_big_bin":          # the active queries of one workgroup: above the 512 of the cooperative bins
            assert nchunk == 1 and c["S"] * (T - c["tstart"]) > 512
        else:
            assert c["B"] == 1 and R * T == 640
    # a bound of zero would ask the kernel for exact float64 results: only where the result is exactly zero (one node: logp = 0)
    for k in rc.outputs(c):
        kind, bd = rc.bound(c, k, r64, r32)
        assert bd > 0 or float(r64[k].abs().max()) == 0.0, k


@pytest.mark.parametrize("mutant,name", [
    ("instance_r_div_S", "ops_pb"), ("tstart_ignored", "ops_pb"), ("idxB_ignored", "ops_pb"),
    ("temp_dropped_in_grad", "temp0.5_M20"), ("tanh_derivative_dropped", "peaked_M20"), ("glimpse_unmasked", "ops_pb"),
    ("entropy_from_unclipped", "peaked_M20"), ("rem_of_previous_step", "ops_dyn_M20"),
])
def test_case_list_sees_the_mutant(mutant, name):
    c = rc.CASES[name]
    op, glogp, r64, r32 = rc.reference(name)
    got = rr.reeval_with_grads(op, glogp, mutant=mutant)
    bad = rc.misses(c, got, r64, r32)
    assert bad, (mutant, name)
    if mutant == "temp_dropped_in_grad":                 # the values are untouched: only gradients may show it
        assert all(k in rr.GRADS for k, *_ in bad)
    if mutant == "entropy_from_unclipped":
        assert [k for k, *_ in bad] == ["entropy"]
    assert set(rr.MUTANTS) == {"instance_r_div_S", "tstart_ignored", "idxB_ignored", "temp_dropped_in_grad",
                               "tanh_derivative_dropped", "glimpse_unmasked", "entropy_from_unclipped", "rem_of_previous_step"}
