"""eamrl_reeval_backward_lp (csrc/reeval.hip: k_reeval_bwd_lp) through ops.ReevalPlan.backward_lp: the gradient with respect to
the folded logit key Lp alone, which is all an adapted logit key needs (EAS-Emb, eam_rl4co_amd/search.py).  Every single-chunk
backward case of tests/reeval_cases.py without a dynamic embedding (rows_*, edge_M* up to 112 nodes, ops_* with / without Pb,
gctx, NC 0 .. 2, the rollout's log-probs or heads handed in, tstart 0 / 1, peaked / clip0 / temp / forced / tie / policy-scale,
the gather cases) against the float64 restatement's dLp (tests/reeval_ref.py) with the bound of tests/reeval_cases.py: MARGIN = 4
times the error of the restatement's own float32 run (1e-4 of the float64 norm in the policy-scale cases).  A node no query can
see keeps dLp exactly zero.

Measured on the MI355X, kernel error / error of the restatement's float32 run (norm of the difference), the largest over the 42
cases and the case it occurs in:
  dLp    3.24  ops_rollout_logp_M20       (the normaliser is recovered from a float32 log-prob there, as in the full backward,
                                           whose dLp has the same figure in the same case: tests/test_gpu_reeval.py)
"""
import pytest
import torch

import reeval_cases as rc
import reeval_ref as rr

pytestmark = pytest.mark.gpu

DEV = "cuda"
LP_CASES = [n for n, c in rc.CASES.items() if c["backward"] and c["M"] <= rr.KEY_CHUNK and not c["dyn"]]


def dev(x):
    return None if x is None else x.to(DEV).contiguous()


def make_plan(name, cache_layout=False, S=None):
    """The plan of case `name` as tests/test_gpu_reeval.py builds it, with lse from a forward pass unless the case hands in the
    rollout's log-probs.  cache_layout: the operands in a decoder cache's slot order (K | V | L | Pa | Pb | Lp), read in place.
    S: only the case's first S starts (rows are in "(s b)" order: its first S * B rows)."""
    from eam_rl4co_amd import ops

    c = rc.CASES[name]
    op, glogp, r64, _ = rc.reference(name)
    logp64 = r64["logp"]
    if S is not None:
        R = S * c["B"]
        op = {k: v[:, :R] if k == "sc" and v is not None else v[:R] if k in ("idxA", "idxB", "mask", "actions", "heads") and v is not None
              else v for k, v in op.items()}
        c, glogp, logp64 = dict(c, S=S), glogp[:R], logp64[:R]
    names = ["K", "V", "Lp", "Pa"] + (["Pb"] if c["pb"] else [])
    slots = None
    if cache_layout:
        order = ["K", "V", "L", "Pa"] + (["Pb"] if c["pb"] else []) + ["Lp"]
        buf = dev(torch.cat([torch.full_like(op["K"], float("nan")) if k == "L" else op[k] for k in order], dim=-1))
        slots = {k: order.index(k) for k in names}
    else:
        buf = dev(torch.cat([op[k] for k in names], dim=-1))
    pack = rr.pack_mask_bits_chunked if c["M"] > rr.KEY_CHUNK else rr.pack_mask_bits
    t0 = c["tstart"]
    fed = logp64.float() if c["rollout_logp"] else None
    plan = ops.ReevalPlan(buf, c["pb"], dev(op["gctx"]), dev(op["Cvec"]), dev(op["idxA"]), dev(op["idxB"]), dev(op["sc"]),
                          dev(pack(op["mask"].numpy())), dev(op["actions"]), c["S"], t0, c["clip"], c["temp"],
                          rollout_logp=dev(fed), rollout_heads=dev(op["heads"][:, t0:]) if c["rollout_heads"] else None,
                          rem=dev(rr.rem_rows(op["rem"])) if c["dyn"] else None, dyn=dev(op["dyn"]), slots=slots, E=rr.E)
    plan.forward()
    assert (plan.lse is None) == c["rollout_logp"]
    return plan, dev(glogp)


@pytest.mark.parametrize("name", LP_CASES)
def test_backward_lp_matches_the_float64_restatement(name):
    c = rc.CASES[name]
    _, _, r64, r32 = rc.reference(name)
    plan, g = make_plan(name)
    got = plan.backward_lp(g).cpu()
    kind, bd = rc.bound(c, "dLp", r64, r32)
    fig = float((got.double() - r64["dLp"]).abs().max()) if kind != "norm" else rc.error("dLp", got, r64)
    f32 = rc.error("dLp", r32["dLp"], r64)
    print(f"EASLP {name} dLp {kind} kernel {fig:.3e} float32-restatement {f32:.3e} ratio {fig / f32 if f32 else float('nan'):.2f} "
          f"bound {bd:.3e} ref {float(r64['dLp'].norm()):.3e}")
    assert got.shape == (c["B"], c["M"], rr.E) and torch.isfinite(got).all()
    for b in range(c["B"]):
        n = rc.dead_node(c, b)
        if n >= 0:
            assert (got[b, n] == 0).all(), (b, n)
    assert rc.misses(c, {"dLp": got}, r64, r32, names=["dLp"]) == []


@pytest.mark.parametrize("name", ["ops_pb", "ops_rollout_heads", "rows_B100_S13_M33_T7"])
def test_backward_lp_accumulates_into_out(name):
    c = rc.CASES[name]
    _, _, r64, r32 = rc.reference(name)
    plan, g = make_plan(name)
    out = torch.zeros(c["B"], c["M"], rr.E, device=DEV)
    assert plan.backward_lp(g, out=out) is out
    plan.backward_lp(g, out=out)
    assert rc.misses(c, {"dLp": out.cpu() / 2}, r64, r32, names=["dLp"]) == []       # (halving is exact)


@pytest.mark.parametrize("name", ["ops_pb", "ops_nc2"])
def test_backward_lp_reads_a_decoder_cache_in_place(name):
    c = rc.CASES[name]
    _, _, r64, r32 = rc.reference(name)
    plan, g = make_plan(name, cache_layout=True)
    assert rc.misses(c, {"dLp": plan.backward_lp(g).cpu()}, r64, r32, names=["dLp"]) == []


@pytest.mark.parametrize("name", ["edge_M113", "ops_dyn_M20"])
def test_backward_lp_refuses_key_chunks_and_the_dynamic_embedding(name):
    c = rc.CASES[name]
    plan, g = make_plan(name)
    out = torch.zeros(c["B"], c["M"], rr.E, device=DEV)
    with pytest.raises(RuntimeError, match="eamrl_reeval_backward_lp"):
        plan.backward_lp(g, out=out)
    torch.cuda.synchronize()
    assert (out == 0).all()          # nothing was launched


@pytest.mark.parametrize("name", ["ops_pb", "ops_rollout_heads", "edge_M33", "edge_M65", "ops_rollout_logp_M65"])
def test_backward_lp_is_the_full_backwards_dLp_bit_for_bit(name):
    """k_reeval_bwd_lp and k_reeval_bwd_logits run the same stages (csrc/reeval_tile.hpp; the full backward writes the logit
    stage out with its extra terms) over the same tiles, so with one start per instance -- nchunk = 1: one workgroup owns an
    instance and every dLp address takes exactly one atomic add, no order to differ in -- the two kernels' dLp are the same bits
    (M = 20, 33, 65: the 2, 4 and 7 key-tile instantiations; the glimpse recomputed, the rollout's heads handed in, the
    normaliser recovered from the rollout's log-probs)."""
    plan, g = make_plan(name, S=1)
    assert plan.nchunk == 1
    E = rr.E
    full = plan.backward(g)[0][..., 2 * E:3 * E]           # (the operands lie K | V | Lp | Pa [| Pb])
    lp = plan.backward_lp(g)
    assert float(full.abs().max()) > 0
    assert torch.equal(lp, full)
