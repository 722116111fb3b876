"""The synthetic cases of the re-evaluation tests (tests/test_host_reeval_ref.py on the CPU, tests/test_gpu_reeval.py on the
GPU): operands from a seeded generator, the float64 / float32 runs of the restatement (tests/reeval_ref.py), computed once per
case and shared, and the bound of every compared output.

Bounds (none comes from the kernels):
  policy-scale cases   logp / lse / entropy within 1e-5 (the contract of include/eamrl.h); every gradient tensor within 1e-4 of
                       its own float64 norm, norm-wise
  every other case     the error of the restatement's float32 run against its float64 run, per case and per output (max-abs for
                       the values, the norm of the difference for a gradient tensor), times FACTOR[output]
  a gradient tensor that is exactly zero in float64: exactly zero where the case says so (`exact_zero`), otherwise max-abs
                       within FACTOR times the largest float32-run max-abs error among the case's gradient tensors
"""
import functools

import torch

import reeval_ref as rr

E = rr.E
VALUES = ("logp", "lse", "entropy")
MARGIN = 4.0           # over a float32-vs-float64 difference, as tests/test_gpu_filter.py
# Kernel error / float32-restatement error allowed per output: MARGIN times RATIO.  RATIO is 1 except for the entropy: the kernels
# form it as lse - (sum e z) / (sum e), three roundings at the magnitude of lse (up to `clip` = 10: half an ulp is 4.8e-7 each)
# plus the cancellation, where the restatement's -sum p (z - lse) carries one (the error of lse shifts every z - lse alike).
# Measured on the MI355X: 4.29 times the float32 restatement's error at the worst case (tie_M20: 1.9e-6 against 4.5e-7, i.e.
# two ulps of lse) -- rounding, inside the 1e-5 of the header; every other output stays below 3.3 (tests/test_gpu_reeval.py).
# dCvec likewise: every workgroup adds its partial sums into the same NC x 128 floats with float atomics (600 workgroups in the
# rows_B100_S13_* cases), a serial sum in arbitrary order whose every add rounds at the size of the running total, where the
# restatement's einsum sums in blocks.  Measured 3.23 and 3.98 times the float32 restatement's error in two runs of
# rows_B100_S13_M20_T7_heads (the order of the atomics differs from run to run); 3.04 at most in every other case.
RATIO = {k: 1.0 for k in VALUES + rr.GRADS}
RATIO["entropy"] = 4.29
RATIO["dCvec"] = 3.98
FACTOR = {k: MARGIN * v for k, v in RATIO.items()}


def _case(name, B, S, M, T, **kw):
    c = dict(name=name, B=B, S=S, M=M, T=T, tstart=1, pb=True, gctx=True, NC=1, dyn=False, rollout_heads=False,
             rollout_logp=False, neg_idx=False, scale="normal", clip=10.0, temp=1.0, forced=False, tie=False, mask="random",
             idx_all=None, backward=True)
    assert not set(kw) - set(c)
    c.update(kw)
    return c


def _build():
    cs = []
    # rows per workgroup: nchunk = max(1, min(S, ceil(512 / B))) workgroups take rows S ch / nchunk .. S (ch + 1) / nchunk
    cs += [_case("rows_B512_S3_M8_T6", 512, 3, 8, 6), _case("rows_B100_S13_M33_T7", 100, 13, 33, 7),
           _case("rows_B64_S9_M20_T19", 64, 9, 20, 19), _case("rows_B100_S13_M113_T5", 100, 13, 113, 5),
           _case("rows_B100_S13_M12_T7_dyn", 100, 13, 12, 7, dyn=True),
           _case("rows_B100_S13_M20_T7_heads", 100, 13, 20, 7, rollout_heads=True)]
    # tile and chunk edges
    for M in (1, 2, 15, 16, 17, 32, 33, 64, 65, 111, 112, 113, 224, 225):
        cs.append(_case(f"edge_M{M}", 2, 3, M, min(M, 9), mask="edges", tstart=0 if M == 1 else 1))
    # operand combinations
    o = dict(B=3, S=4, M=20, T=9)
    cs += [_case("ops_pb", **o), _case("ops_nopb", **o, pb=False), _case("ops_nogctx", **o, gctx=False),
           _case("ops_nc0", **o, NC=0), _case("ops_nc2", **o, NC=2), _case("ops_nc3_fwd", **o, NC=3, backward=False),
           _case("ops_nc4_fwd", **o, NC=4, backward=False), _case("ops_negidx", **o, neg_idx=True),
           _case("ops_tstart0", **o, tstart=0), _case("ops_rollout_logp_M20", **o, rollout_logp=True),
           _case("ops_rollout_logp_M65", 3, 4, 65, 9, rollout_logp=True), _case("ops_rollout_heads", **o, rollout_heads=True),
           _case("ops_dyn_M20", **o, dyn=True), _case("ops_dyn_M130", 3, 4, 130, 9, dyn=True)]
    # distribution shapes
    for M in (20, 65, 130):
        d = dict(B=3, S=4, M=M, T=9)
        cs += [_case(f"peaked_M{M}", **d, scale="peaked"), _case(f"clip0_M{M}", **d, clip=0.0),
               _case(f"temp0.5_M{M}", **d, temp=0.5), _case(f"temp2_M{M}", **d, temp=2.0),
               _case(f"forced_M{M}", **d, forced=True), _case(f"tie_M{M}", **d, tie=True),
               _case(f"policy_M{M}", **d, scale="policy")]
    # the gather kernel: 640 queries on one bin (above the 512 of its cooperative path); no index at all
    cs += [_case("gather_one_bin", 1, 40, 8, 16, idx_all=5), _case("gather_no_index", 1, 40, 8, 16, idx_all=-1)]
    # (those two get nchunk = 40 workgroups of 16 queries each.)  The gather's cooperative bins need more than 512 queries of ONE
    # workgroup on a node, hence nchunk = 1 (B >= 512): three rows of 172 steps, 513 active queries of a workgroup on node 5
    cs += [_case("gather_big_bin", 512, 3, 8, 172, idx_all=5, pb=False)]
    return {c["name"]: c for c in cs}


CASES = _build()
NAMES = list(CASES)
EDGE_NODES = sorted({e + d for e in range(16, 1024, 16) for d in (-1, 0)})      # both sides of every 16-key tile / 32-bit word
FORCED_EVERY, TIE_EVERY = (3, 2), (3, 1)        # steps t with t % 3 == 2 are forced, with t % 3 == 1 ties
SCALES = {"normal": (1.0, 2.0, 1.0), "peaked": (5.0, 8.0, 1.6), "policy": (0.3, 0.25, 1.0)}      # of K, Lp and the query parts


def dead_node(c, b):
    """The node of instance b that is never feasible (none below four nodes)."""
    return (7 * b + 3) % c["M"] if c["M"] >= 4 else -1


def unindexed_node(c):
    """The node that idxA / idxB never name (none below four nodes)."""
    return 2 if c["M"] >= 4 and c["idx_all"] is None else -1


def tie_nodes(c):
    return (0, c["M"] - 2)       # (never a dead node: see operands)


def operands(name):
    """-> (op, glogp): the operands as reeval_ref.reeval takes them (float32 tensors), the upstream gradient [R, T]."""
    c = CASES[name]
    g = torch.Generator().manual_seed(1000 + NAMES.index(name))
    B, S, M, T = c["B"], c["S"], c["M"], c["T"]
    R = B * S

    def randn(*shape, s=1.0):
        return torch.randn(*shape, generator=g) * s

    ks, ls, qs = SCALES[c["scale"]]
    op = dict(K=randn(B, M, E, s=ks), V=randn(B, M, E), Lp=randn(B, M, E, s=ls), Pa=randn(B, M, E, s=0.7 * qs),
              Pb=randn(B, M, E, s=0.5 * qs) if c["pb"] else None, gctx=randn(B, E, s=0.5 * qs) if c["gctx"] else None,
              Cvec=randn(c["NC"], E, s=0.5) if c["NC"] else None, sc=torch.rand(c["NC"], R, T, generator=g) if c["NC"] else None,
              S=S, tstart=c["tstart"], clip=c["clip"], temp=c["temp"], rem=None, dyn=None, heads=None)
    inst = torch.arange(R) % B
    # masks: a random feasible set per (row, step); `edges` toggles the nodes at both sides of every tile / word boundary
    mask = torch.rand(R, T, M, generator=g) < 0.6
    if c["mask"] == "edges":
        e = torch.tensor([n for n in EDGE_NODES if n < M], dtype=torch.long)
        if len(e):
            par = (torch.arange(R)[:, None, None] + torch.arange(T)[None, :, None] + torch.arange(len(e))[None, None, :]) % 2
            mask[:, :, e] = par == 0
    n1, n2 = tie_nodes(c)
    if c["tie"]:                                 # two nodes with bit-identical rows, masked alike at every step
        for X in (op["K"], op["V"], op["Lp"]):
            X[:, n2] = X[:, n1]
        mask[:, :, n2] = mask[:, :, n1]
    alive = torch.ones(R, M, dtype=torch.bool)
    for b in range(B):
        if dead_node(c, b) >= 0:
            alive[inst == b, dead_node(c, b)] = False
    if c["tie"]:
        assert alive[:, n1].all() and alive[:, n2].all()
    mask &= alive[:, None, :]
    free = alive.clone()
    if c["tie"]:
        free[:, [n1, n2]] = False                # (the tie nodes are chosen at the tie steps only: their gradient rows stay equal)
    pick = torch.multinomial(free.float(), T, replacement=True, generator=g)          # [R, T]: an alive node per step
    mask.scatter_(2, pick[..., None], True)      # no step with an empty mask
    if c["mask"] == "edges" and M > rr.KEY_CHUNK:        # step 2: all feasible nodes in the last chunk; step 3: in the first one
        last = rr.KEY_CHUNK * ((M - 1) // rr.KEY_CHUNK)
        mask[:, 2, :last] = False
        mask[:, 2, last] = True
        mask[:, 3, rr.KEY_CHUNK:] = False
        mask[:, 3, 1] = True
    t = torch.arange(T)
    if c["forced"]:
        f = t % FORCED_EVERY[0] == FORCED_EVERY[1]
        mask[:, f] = False
        mask[:, f] = mask[:, f].scatter(2, pick[:, f, None], True)
    if c["tie"]:
        f = t % TIE_EVERY[0] == TIE_EVERY[1]
        mask[:, f] = False
        mask[:, f, n1] = mask[:, f, n2] = True
    w = mask.float()
    if c["tie"]:
        w[:, ~f, n1] = w[:, ~f, n2] = 0.0
    actions = torch.multinomial(w.reshape(R * T, M), 1, generator=g).reshape(R, T)
    op["mask"], op["actions"] = mask, actions

    def indices():
        if c["idx_all"] is not None:
            return torch.full((R, T), c["idx_all"], dtype=torch.int32)
        idx = torch.randint(0, M, (R, T), generator=g)
        if unindexed_node(c) >= 0:
            idx[idx == unindexed_node(c)] = 0
        if c["neg_idx"]:
            idx[torch.rand(R, T, generator=g) < 1 / 3] = -1
        return idx.to(torch.int32)

    op["idxA"] = indices()
    op["idxB"] = (torch.full((R, T), -1, dtype=torch.int32) if c["idx_all"] is not None else indices()) if c["pb"] else None
    if c["dyn"]:
        op["rem"] = torch.rand(R, T, M, generator=g)
        op["dyn"] = randn(3, E, s=0.5) * torch.tensor([1.0, 1.0, ls])[:, None]
    glogp = randn(R, T)
    return op, glogp


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (op, glogp, r64, r32): the float64 and float32 runs of the restatement (with gradients unless the case is forward
    only).  A case with `rollout_heads` hands the restatement the float32-rounded float64 heads, as the kernel gets them.
    Computed once; nothing may modify it."""
    c = CASES[name]
    op, glogp = operands(name)
    run = rr.reeval_with_grads if c["backward"] else (lambda o, _, dtype: {k: v.detach() for k, v in rr.reeval(rr.cast(o, dtype)).items()})
    if c["rollout_heads"]:
        op["heads"] = rr.reeval(rr.cast(op, torch.float64))["heads"].float()
    return op, glogp, run(op, glogp, dtype=torch.float64), run(op, glogp, dtype=torch.float32)


def outputs(c):
    """The outputs compared in case c."""
    out = ["logp"] + ([] if c["rollout_logp"] else ["lse", "entropy"])         # (rollout log-probs: no forward pass, lse = None)
    if c["backward"]:
        out += ["dK", "dV", "dLp", "dPa"] + (["dPb"] if c["pb"] else []) + (["dgctx"] if c["gctx"] else []) + \
               (["dCvec"] if c["NC"] else []) + (["ddyn"] if c["dyn"] else [])
    return out


def exact_zero(c):
    """Gradient tensors the kernels never write in case c."""
    z = ("dPa", "dPb") if c["idx_all"] == -1 else ("dPb",) if c["idx_all"] is not None else ()
    return tuple(k for k in z if k != "dPb" or c["pb"])


def error(name, got, r64):
    """The error figure of output `name`: max-abs for a value, the norm of the difference for a gradient tensor."""
    d = got.double() - r64[name]
    return float(d.abs().max()) if name in VALUES else float(d.norm())


def bound(c, name, r64, r32):
    """-> (kind, bound) of output `name` of case c; kind: "maxabs", "norm", or "zero" (max-abs of a tensor that is exactly zero
    in float64)."""
    grads = [k for k in outputs(c) if k in rr.GRADS]
    if name in rr.GRADS and float(r64[name].abs().max()) == 0.0:
        if name in exact_zero(c):
            return "zero", 0.0
        return "zero", FACTOR[name] * max(float((r32[k].double() - r64[k]).abs().max()) for k in grads)
    if c["scale"] == "policy":
        return ("maxabs", 1e-5) if name in VALUES else ("norm", 1e-4 * float(r64[name].norm()))
    return ("maxabs" if name in VALUES else "norm"), FACTOR[name] * error(name, r32[name], r64)


def misses(c, got, r64, r32, names=None):
    """[(output, kind, figure, bound)] of the compared outputs of `got` that lie beyond their bound."""
    bad = []
    for name in names or outputs(c):
        kind, bd = bound(c, name, r64, r32)
        fig = float((got[name].double() - r64[name]).abs().max()) if kind != "norm" else error(name, got[name], r64)
        if not fig <= bd:
            bad.append((name, kind, fig, bd))
    return bad
