"""eamrl_reeval_backward with an entropy upstream gradient (eamrl_reeval.gent, csrc/reeval.hip: k_reeval_bwd_logits<.., ENT>)
through ops.ReevalPlan.backward(glogp, gent), every gradient tensor on its own against the float64 run of the restatement
(tests/reeval_ref.py):  d/d(operands) of  sum(glogp * logp) + sum(gent * entropy).

The restatement hands its entropy back detached, so `with_entropy_grads` forms the same expression once more from the `u`
(raw logits, with their graph) that `reeval_ref.reeval` returns -- z = clip tanh(u) / temp over the feasible nodes,
H = -sum p log p -- and asserts that its value IS the restatement's entropy before differentiating it.

Cases: those of tests/reeval_cases.py that the native entropy gradient serves (single-chunk graphs), operands and glogp as there;
gent from its own seeded generator at the scale of glogp.  Bounds: the rule of reeval_cases.bound -- error against float64 at
most MARGIN (4) x RATIO[output] x the error of the restatement's float32 run, per case and per output (norm of the difference);
policy-scale cases 1e-4 of the float64 norm; a tensor that is exactly zero in float64 as there.  None comes from the kernels.

RATIO is 1 for every gradient tensor: measured on the MI355X, none exceeds the margin (the figures are next to RATIO below).
"""
import functools
import math

import pytest
import torch

import reeval_cases as rc
import reeval_ref as rr

pytestmark = pytest.mark.gpu

DEV = "cuda"

CASES = ["ops_pb", "ops_nopb", "ops_nogctx", "ops_nc0", "ops_nc2", "ops_tstart0", "ops_rollout_heads", "ops_dyn_M20"] + \
        [f"edge_M{M}" for M in (2, 15, 16, 17, 32, 33, 64, 65, 111, 112)] + \
        ["tie_M20", "forced_M20", "clip0_M20", "temp0.5_M20", "peaked_M65", "policy_M20", "policy_M65",
         "rows_B100_S13_M33_T7", "rows_B64_S9_M20_T19"]

# kernel error / float32-restatement error per gradient tensor: bound = rc.MARGIN * RATIO * (float32-restatement error)
RATIO = {k: 1.0 for k in rr.GRADS}

# MEASURED on the MI355X (the prints of test_entropy_backward_matches_the_float64_restatement): the largest ratio per tensor over
# the 27 cases and the case it occurs in -- all inside the margin of 4, so every RATIO stays 1:
#   dK 1.25 ops_pb         dV 2.07 edge_M2        dLp 1.87 policy_M20    dPa 1.59 temp0.5_M20    dPb 1.60 edge_M2
#   dgctx 1.73 policy_M20  dCvec 3.33 rows_B64_S9_M20_T19 (float atomics of 512 workgroups on NC x 128 floats, as in
#   reeval_cases.py; the order differs from run to run)            ddyn 1.47 ops_dyn_M20


def gent_of(name):
    c = rc.CASES[name]
    g = torch.Generator().manual_seed(7000 + rc.NAMES.index(name))
    return torch.randn(c["B"] * c["S"], c["T"], generator=g)


def entropy_with_graph(op, out):
    """reeval_ref.reeval's entropy (lines "z = clip tanh(u)" .. "entropy") from its graph-carrying raw logits out["u"]."""
    u, active = out["u"], out["active"]
    mask = op["mask"] | ~active[:, :, None]
    z = op["clip"] * torch.tanh(u) if op["clip"] > 0 else u
    zt = (z / op["temp"]).masked_fill(~mask, -math.inf)
    logpn = zt - torch.logsumexp(zt, dim=-1)[..., None]
    # (the infeasible entries are taken out BEFORE the product: where() after exp(-inf) * -inf would hand NaN to autograd)
    lp = torch.where(mask, logpn, torch.zeros_like(logpn))
    ent = -torch.where(mask, lp.exp() * lp, torch.zeros_like(lp)).sum(-1)
    ent = torch.where(active, ent, torch.zeros_like(ent))
    assert torch.equal(ent.detach(), out["entropy"])          # the restatement's own entropy, bit for bit
    return ent


def with_entropy_grads(op, glogp, gent, dtype):
    """Autograd gradients of sum(glogp * logp) + sum(gent * entropy) of rr.reeval with every operand in `dtype`."""
    op = rr.cast(op, dtype)
    leaves = {}
    for g, name in rr.DIFF:
        if op.get(name) is not None:
            op[name] = op[name].detach().clone().requires_grad_()
            leaves[g] = op[name]
    out = rr.reeval(op)
    ent = entropy_with_graph(op, out)
    ((glogp.to(dtype) * out["logp"]).sum() + (gent.to(dtype) * ent).sum()).backward()
    res = {"entropy": ent.detach(), "active": out["active"]}
    for g, leaf in leaves.items():
        res[g] = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
    return res


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (op, glogp, gent, r64, r32), computed once per case; nothing may modify it."""
    op, glogp, _, _ = rc.reference(name)          # (a rollout-heads case: with the float32-rounded float64 heads, as there)
    gent = gent_of(name)
    return op, glogp, gent, with_entropy_grads(op, glogp, gent, torch.float64), with_entropy_grads(op, glogp, gent, torch.float32)


def grad_names(c):
    return [k for k in rc.outputs(c) if k in rr.GRADS]


def make_plan(name, want_entropy=True, rollout_logp=None):
    from eam_rl4co_amd import ops

    c = rc.CASES[name]
    op = rc.reference(name)[0]

    def dev(x):
        return None if x is None else x.to(DEV).contiguous()

    names = ["K", "V", "Lp", "Pa"] + (["Pb"] if c["pb"] else [])
    buf = dev(torch.cat([op[k] for k in names], dim=-1))
    pack = rr.pack_mask_bits_chunked if c["M"] > rr.KEY_CHUNK else rr.pack_mask_bits
    t0 = c["tstart"]
    plan = ops.ReevalPlan(buf, c["pb"], dev(op["gctx"]), dev(op["Cvec"]), dev(op["idxA"]), dev(op["idxB"]), dev(op["sc"]),
                          dev(pack(op["mask"].numpy())), dev(op["actions"]), c["S"], t0, c["clip"], c["temp"],
                          want_entropy=want_entropy, rollout_logp=dev(rollout_logp),
                          rollout_heads=dev(op["heads"][:, t0:]) if c["rollout_heads"] else None,
                          rem=dev(rr.rem_rows(op["rem"])) if c["dyn"] else None, dyn=dev(op["dyn"]))
    return plan, names


def run_backward(name, glogp, gent, nchunk=None):
    """-> dict of the kernels' gradient tensors (CPU) for case `name`; gent None: the call without the field."""
    c = rc.CASES[name]
    plan, names = make_plan(name)
    if nchunk is not None:
        plan.nchunk = nchunk
    plan.forward()
    dbuf, dg, dc = plan.backward(glogp.to(DEV), None if gent is None else gent.to(DEV))
    got = {"d" + k: dbuf[..., i * rr.E:(i + 1) * rr.E].cpu() for i, k in enumerate(names)}
    if dg is not None:
        got["dgctx"] = dg.cpu()
    if dc is not None:
        got["dCvec"] = dc.cpu()
    if c["dyn"]:
        got["ddyn"] = plan.ddyn.cpu()
    got["entropy"] = plan.entropy.cpu()
    torch.cuda.synchronize()
    return got


def bound(c, k, r64, r32):
    kind, bd = rc.bound(c, k, r64, r32)             # (MARGIN * reeval_cases.RATIO[k] * float32 error, or the fixed policy bound)
    if c["scale"] != "policy":
        bd = bd / rc.RATIO[k] * RATIO[k]            # this module's own ratios, all of which start at 1
    return kind, bd


@pytest.mark.parametrize("name", CASES)
def test_entropy_backward_matches_the_float64_restatement(name):
    c = rc.CASES[name]
    assert c["M"] <= rr.KEY_CHUNK and c["backward"] and not c["rollout_logp"]
    op, glogp, gent, r64, r32 = reference(name)
    got = run_backward(name, glogp, gent)
    names = grad_names(c)
    bad = []
    for k in names:                              # each figure before any assert
        kind, bd = bound(c, k, r64, r32)
        fig = float((got[k].double() - r64[k]).abs().max()) if kind != "norm" else rc.error(k, got[k], r64)
        f32 = rc.error(k, r32[k], r64)
        print(f"ENTBWD {name} {k} {kind} kernel {fig:.3e} float32-restatement {f32:.3e} ratio {fig / f32 if f32 else float('nan'):.2f} "
              f"bound {bd:.3e} ref {float(r64[k].norm()):.3e}")
        if not fig <= bd:
            bad.append((k, kind, fig, bd))
    assert all(torch.isfinite(got[k]).all() for k in got)
    for b in range(c["B"]):                     # nodes no query can see: untouched by the entropy term too
        n = rc.dead_node(c, b)
        if n >= 0:
            assert all((got[k][b, n] == 0).all() for k in ("dK", "dV", "dLp")), (b, n)
    # the entropy term is really there: the float64 gradient differs from the one without it
    base = rc.reference(name)[2]
    assert any(float((r64[k] - base[k]).norm()) > 1e-3 * float(base[k].norm()) for k in names)
    assert bad == []


def single_query_picks(c):
    """Six (row, step) positions with step >= tstart: first and last query, and rows of different instances and start groups."""
    R, T, t0 = c["B"] * c["S"], c["T"], c["tstart"]
    return [(0, t0), (R - 1, T - 1), (R // 2, (t0 + T) // 2), (1, T - 1), (R - 2, t0), (c["B"] + 1, min(t0 + 2, T - 1))]


@pytest.mark.parametrize("name", ["ops_pb", "ops_nopb", "ops_rollout_heads", "ops_dyn_M20", "edge_M33", "edge_M65", "forced_M20"])
def test_zero_entropy_gradient_equals_no_entropy_gradient(name):
    """gent = zeros gives the bits of gent = None.  Two calls of the backward are comparable bit for bit only where no address
    receives more than one non-zero float atomic: the kernels add their partial sums with atomics in whatever order the
    workgroups and wavefronts arrive (two calls with gent = None differ in the last bits of every tensor at the default row
    split, and of dPa dPb dgctx dCvec ddyn at any: measured on the MI355X, 3 of 3 repeats).  So the comparison is made where it
    is exact by construction, with torch.equal on every gradient tensor:
      (a) glogp non-zero at ONE (row, step): every other query contributes exact zeros, every address gets at most one
          non-zero add -- all tensors, six positions per case;
      (b) the full glogp with one workgroup per instance (nchunk = 1): dK dV dLp are register sums of a workgroup in tile order,
          added once per address -- all queries at once."""
    c = rc.CASES[name]
    glogp = rc.reference(name)[1]
    for r, t in single_query_picks(c):
        g1 = torch.zeros_like(glogp)
        g1[r, t] = glogp[r, t]
        none = run_backward(name, g1, None)
        zero = run_backward(name, g1, torch.zeros_like(glogp))
        for k in grad_names(c):
            assert torch.equal(zero[k], none[k]), (k, r, t)
    none = run_backward(name, glogp, None, nchunk=1)
    zero = run_backward(name, glogp, torch.zeros_like(glogp), nchunk=1)
    assert float(none["dK"].abs().max()) > 0
    for k in ("dK", "dV", "dLp"):
        assert torch.equal(zero[k], none[k]), k


@pytest.mark.parametrize("name", ["forced_M20", "ops_pb"])
def test_entropy_gradient_of_forced_and_inactive_steps_is_exactly_zero(name):
    """gent only at steps with a single feasible node (H = 0, p = 1) and at t < tstart, glogp = 0: every gradient exactly zero."""
    c = rc.CASES[name]
    op, glogp = rc.reference(name)[:2]
    single = op["mask"].sum(-1) == 1
    inactive = (torch.arange(c["T"]) < c["tstart"])[None, :].expand_as(single)
    where = single | inactive
    assert inactive.any() and (name != "forced_M20" or (single & ~inactive).any())
    gent = torch.where(where, 3.0 + torch.rand(where.shape, generator=torch.Generator().manual_seed(3)), torch.zeros(()))
    got = run_backward(name, torch.zeros_like(glogp), gent)
    assert (got["entropy"][where] == 0).all()
    for k in grad_names(c):
        assert torch.isfinite(got[k]).all() and (got[k] == 0).all(), k


def test_entropy_gradient_is_refused_where_it_is_not_built():
    """Key chunks (M > 112), and a plan whose forward wrote no entropy: -1 before any launch, nothing written."""
    name = "edge_M113"
    plan, _ = make_plan(name)
    plan.forward()
    glogp = rc.reference(name)[1].to(DEV)
    with pytest.raises(RuntimeError, match="p->M <= 112"):
        plan.backward(glogp, torch.ones_like(glogp))
    dbuf, _, _ = plan.backward(glogp)            # the same plan still serves the backward without the field
    assert torch.isfinite(dbuf).all()
    plan, _ = make_plan("ops_pb", want_entropy=False)
    plan.forward()
    glogp = rc.reference("ops_pb")[1].to(DEV)
    with pytest.raises(ValueError, match="want_entropy"):
        plan.backward(glogp, torch.ones_like(glogp))


def test_a_plan_with_the_rollouts_log_probs_still_serves_the_entropy_gradient():
    """want_entropy=True runs the forward kernel whatever else the plan was given: handed the rollout's log-probs as well, the
    backward with gent reads the normaliser that pass wrote (not one recovered from the log-probs) -- the bits of the plain plan
    in the tensors that one workgroup per instance adds once per address."""
    name = "ops_pb"
    op, glogp, gent, r64, _ = reference(name)
    res = []
    for fed in (None, rc.reference(name)[2]["logp"].float()):
        plan, _ = make_plan(name, rollout_logp=fed)
        plan.nchunk = 1
        logp = plan.forward()
        assert fed is None or (plan.lse is None and not torch.equal(logp.cpu(), fed))      # the kernel's values, not the ones handed in
        dbuf, _, _ = plan.backward(glogp.to(DEV), gent.to(DEV))
        res.append((logp.cpu(), plan.entropy.cpu(), dbuf[..., :3 * rr.E].cpu()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
