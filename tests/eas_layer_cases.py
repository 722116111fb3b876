"""The synthetic cases of the EAS-Lay kernel tests (tests/test_host_eas_lay.py on the CPU, tests/test_gpu_eas_lay_kernel.py on
the GPU).  The operands -- Lp, masks, actions, glogp and the restatement's own heads -- are those of single-chunk, non-dynamic
cases of tests/reeval_cases.py, made by ITS generator (`reeval_cases.operands`, handed this module's shapes for the duration of
the call; that module is left as it was); the layer weights come from a seeded generator here, with non-zero W2.

Shapes: the smallest that reach each code path of k_eas_layer_bwd / the layer rollout -- M 20 (2 key tiles), 33 and 64 (4), 65
and 112 (7); 2, 16, 17 and 128 rows per instance; B 1 (several row chunks), 3 and 100 (nchunk = 1: tiles that straddle rows);
tstart 0 and 1; clip 0 and 10; temperature 1 and 0.7; the normaliser given (lse) and recovered from log-probs; steps with a
single feasible node.

ReLU guard.  relu's kink makes the gradient discontinuous in pre, so a float32 evaluation whose rounding flips the sign of one
pre would differ from float64 by a whole term, not by rounding.  Every case therefore satisfies
    min |pre64| over the live steps  >=  GUARD * max |pre32 - pre64|,   GUARD = 64,
pre32 the float32 restatement's.  The weight seed of a case is walked on the CPU (`walk_seed`) until it holds and recorded in
SEEDS; tests/test_host_eas_lay.py re-checks every case, so no float32 evaluation order can flip a sign and no element needs
excluding.  (b1 is drawn away from zero -- +-[0.9, 1.5], two to three standard deviations of h W1 -- so that the walk is short: with pre centred on zero, the smallest of
10^5 values sits within a few ulps of it.)

Bounds: reeval_cases' rule -- MARGIN = 4 times the float32 restatement's own error against float64, the norm of the difference
per gradient tensor; log-probs within 1e-5 (the header's contract)."""
import functools
from unittest import mock

import torch

import eas_layer_ref as er
import reeval_cases as rc
import reeval_ref as rr

E = er.E
MARGIN = rc.MARGIN
GUARD = 64.0


def _case(name, B, S, M, T, lse, nchunk=None, **kw):
    c = rc._case(name, B, S, M, T, rollout_heads=True, **kw)
    assert M <= rr.KEY_CHUNK and not c["dyn"]
    c["lse"], c["nchunk"] = lse, nchunk         # lse: given to the kernel (True) or recovered from the log-probs (False)
    return c


CASES = {c["name"]: c for c in [
    _case("lay_M20_S2_B3", 3, 2, 20, 9, lse=False),
    _case("lay_M33_S16_B3", 3, 16, 33, 7, lse=True),
    _case("lay_M64_S17_B3_tstart0_clip0", 3, 17, 64, 7, lse=True, nchunk=2, tstart=0, clip=0.0),
    _case("lay_M65_S128_B1_temp0.7", 1, 128, 65, 5, lse=False, temp=0.7),
    _case("lay_M112_S4_B3_forced", 3, 4, 112, 9, lse=True, forced=True),
    _case("lay_M112_S4_B3_forced_logp", 3, 4, 112, 9, lse=False, forced=True),
    _case("lay_M20_S5_B100_nchunk1", 100, 5, 20, 4, lse=False, nchunk=1),
]}
NAMES = list(CASES)
# weight seeds found by walk_seed (the first seed from 0 that meets the ReLU guard)
SEEDS = {'lay_M20_S2_B3': 0, 'lay_M33_S16_B3': 0, 'lay_M64_S17_B3_tstart0_clip0': 0, 'lay_M65_S128_B1_temp0.7': 0,
         'lay_M112_S4_B3_forced': 0, 'lay_M112_S4_B3_forced_logp': 0, 'lay_M20_S5_B100_nchunk1': 6}


def operands(name):
    """-> (op, glogp) of reeval_cases' generator for this module's case `name`."""
    c = CASES[name]
    with mock.patch.dict(rc.CASES, {name: c}), mock.patch.object(rc, "NAMES", rc.NAMES + [name]):
        return rc.operands(name)


def weights(name, seed):
    """Layer weights of the reference's shapes: W1, W2 [B, E, E], b1, b2 [B, E], float32."""
    B = CASES[name]["B"]
    g = torch.Generator().manual_seed(50_000 + 1000 * NAMES.index(name) + seed)
    W1 = torch.randn(B, E, E, generator=g) * 0.1
    sign = torch.where(torch.rand(B, E, generator=g) < 0.5, -1.0, 1.0)
    b1 = sign * (0.9 + 0.6 * torch.rand(B, E, generator=g))
    return dict(W1=W1, b1=b1, W2=torch.randn(B, E, E, generator=g) * 0.05, b2=torch.randn(B, E, generator=g) * 0.1)


def guard_figures(op, lay, heads):
    """-> (min |pre64| over the live steps, max |pre32 - pre64|)."""
    f64 = er.forward(rr.cast(op, torch.float64), er.cast(lay, torch.float64), heads.double())
    f32 = er.forward(rr.cast(op, torch.float32), lay, heads)
    live = f64["active"]
    return float(f64["pre"][live].abs().min()), float((f32["pre"].double() - f64["pre"])[live].abs().max())


def heads_of(op):
    """The restatement's own glimpse outputs, rounded to float32 as the kernel gets them [R, T, E]."""
    o = dict(op)
    o["heads"] = None
    return rr.reeval(rr.cast(o, torch.float64))["heads"].float()


def walk_seed(name, limit=200):
    op, _ = operands(name)
    heads = heads_of(op)
    for seed in range(limit):
        lo, err = guard_figures(op, weights(name, seed), heads)
        if lo >= GUARD * err:
            return seed
    raise AssertionError(f"{name}: no weight seed below {limit} meets the ReLU guard")


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (op, glogp, lay, heads, r64, r32): operands, float32 layer weights, heads [R, T, E] float32, and the float64 / float32
    runs of the restatement with gradients.  Computed once; nothing may modify it."""
    op, glogp = operands(name)
    heads = heads_of(op)
    lay = weights(name, SEEDS[name])
    return op, glogp, lay, heads, er.with_grads(op, lay, heads, glogp, torch.float64), er.with_grads(op, lay, heads, glogp, torch.float32)


def bound(name, grad, r64, r32):
    """MARGIN times the float32 restatement's own error, by norm."""
    return MARGIN * float((r32[grad].double() - r64[grad]).norm())


if __name__ == "__main__":          # python tests/eas_layer_cases.py: the seeds to record in SEEDS
    print({n: walk_seed(n) for n in NAMES})
