"""The cases of the HAM tests (tests/test_host_ham.py on the CPU, tests/test_gpu_ham.py on the GPU): shapes, operands from a
seeded generator, the float64 / float32 runs of the restatement (tests/ham_ref.py), computed once per case and shared, and the
bound of every compared output.

Kernels: ops.hetero_mha (k_hetero_mha, fp32 MFMA) and ops.hetero_mha_backward (k_hetero_mha_bwd), csrc/hetero_attn.hip.

Shapes.  M = 2P + 1 nodes, E = 128, H = 8.  The forward works in tiles of 16 keys / 16 query rows, two key tiles per trip:
  3, 5     one tile; the depot, pickups and deliveries share it (both role chains in tile 0)
  17       two tiles, the second holds one key (P = 8: roles split inside tile 0)
  21, 33   PDP-20 / 32; 33: three tiles, an odd tile count (the clamped second tile of the last trip), P = 16 ends tile 0 + 1 key
  101      PDP-100: P = 50 straddles tile 3;  129: PDP-128, P = 64: the first delivery is the first key of tile 4 + 1
  513      the stated upper bound (EAMRL_HETERO_MHA_MAX_NODES): 33 tiles, 67,584 bytes of LDS (the raised attribute), B = 2
The backward (thread per row / per key, M <= 129 = EAMRL_HETERO_MHA_BWD_MAX_NODES) runs the same shapes up to 129.

Data kinds:
  normal   randn * 1.5 in all six projections
  peak     randn * 0.1, plus a shared direction in every head that lifts the general score of ONE key (node P, the last pickup) 60
           above the rest for every row: every other weight is exp(-60) of it
  equal    all four queries zero: every one of the 2M (depot: M) scores is exactly 0, the softmax is uniform
  pair_high, same_high   randn * 0.1, plus a shared direction in every head of ALL keys and of qpair (pair_high) or qsame
           (same_high): the pair score, or every same-role score, of a non-depot row sits 100 above its general scores (which
           move by +-1).  exp(100) is not a float32: a row maximum taken over the general scores alone overflows here, so these
           cases hold "the maximum over all four groups before any exp".  pair_high: the row's output is its partner's value

Bounds (none comes from the kernels): the protocol of tests/train_cases.py.  The error of an output against the float64 run is
the max-abs difference for the value (y) and the norm of the difference for the gradient (dproj).  It may be at most MARGIN (4,
reeval_cases.MARGIN) times RATIO[output, kind] (1 unless recorded below with its case and arithmetic) times the larger of
  - the same error figure of the restatement's float32 run, and
  - the floor U = 2^-24 times the largest |value| of the output in float64.

Embeddings of the whole encoder (test_gpu_ham.py against ham_embed_pdp20): MARGIN times EMBED_F32_DISTANCE, the max-abs distance
of the float32 run of ham_ref.encoder from the recorded (float32, reference) embeddings, measured on the CPU (one thread):
1.19e-6 with batch norm in eval mode (3 layers) and 2.15e-6 with instance norm (6 layers) at |embedding| <= 4.6; the float64 run
is 1.4e-6 away (the recorded values are the reference's float32).  test_host_ham.py holds the constants to the measurement.
"""
import functools
import json
import os

import numpy as np
import torch

import goldweights
import ham_ref
from _util import GOLDEN
from reeval_cases import MARGIN        # 4.0: over a float32-vs-float64 difference

U = 2.0 ** -24
E, H = 128, 8
MAX_NODES, BWD_MAX_NODES = 513, 129     # include/eamrl.h: EAMRL_HETERO_MHA_MAX_NODES, EAMRL_HETERO_MHA_BWD_MAX_NODES
FWD_SIZES = (3, 5, 17, 21, 33, 101, 129)
RATIO = {}                              # (output, kind) -> measured ratio above 1, with its case and the arithmetic; none so far
EMBED_F32_DISTANCE = {"batch": 1.1920928955078125e-06, "instance": 2.1457672119140625e-06}
MHA_FIXTURES = ("ham_mha_m3", "ham_mha_m5", "ham_mha_m21", "ham_mha_m33")
ROLLOUT_FIXTURES = ("ham_pdp4_greedy", "ham_pdp20_greedy", "ham_pdp20_sampling", "ham_pomo_pdp20_multistart_greedy",
                    "ham_pdp100_greedy", "ham_pdp128_greedy")
POMO = dict(num_encoder_layers=6, normalization="instance", use_graph_context=False)

with open(os.path.join(GOLDEN, "state_dict_contract_ham.json")) as _f:
    CONTRACT = json.load(_f)


def weights(cfg):
    """{key: float32 ndarray} of the closed-form weights for the contract configs "am" / "pomo"."""
    sd = {}
    for k, shape, dt in CONTRACT[cfg]:
        if dt == "float32":
            v = goldweights.tensor_for(k, shape)
            if v is not None:
                sd[k] = v
    return sd


def cfg_for(fx):
    return "pomo" if "policy_kw_num_encoder_layers" in fx else "am"


def _build():
    cs = {}
    for M in FWD_SIZES:
        for B in (1, 3):
            cs[f"M{M}_B{B}"] = dict(M=M, B=B, kind="normal", bwd=True)
    cs[f"M{MAX_NODES}_B2"] = dict(M=MAX_NODES, B=2, kind="normal", bwd=False)
    for M in (21, 101):
        cs[f"M{M}_B2_peak"] = dict(M=M, B=2, kind="peak", bwd=True)
        cs[f"M{M}_B2_equal"] = dict(M=M, B=2, kind="equal", bwd=True)
    for M in (21, 101):                 # (appended: the operands' seeds follow the position in this list)
        cs[f"M{M}_B2_pair_high"] = dict(M=M, B=2, kind="pair_high", bwd=True)
        cs[f"M{M}_B2_same_high"] = dict(M=M, B=2, kind="same_high", bwd=True)
    return cs


CASES = _build()
NAMES = list(CASES)
BWD_NAMES = [n for n in NAMES if CASES[n]["bwd"]]


def operands(name):
    """-> dict(proj [B, M, 6E], dout [B, M, E]) float32 CPU tensors."""
    c = CASES[name]
    g = torch.Generator().manual_seed(5000 + NAMES.index(name))
    B, M = c["B"], c["M"]
    P = (M - 1) // 2
    if c["kind"] == "normal":
        proj = torch.randn(B, M, 6 * E, generator=g) * 1.5
    elif c["kind"] == "peak":
        proj = torch.randn(B, M, 6 * E, generator=g) * 0.1
        lift = 240.0 ** 0.5                             # c * lift * lift = 0.25 * 240 = 60
        proj[:, :, 0:E:E // H] += lift                  # q: component 0 of every head
        proj[:, P, E:2 * E:E // H] += lift              # k of node P
    elif c["kind"] in ("pair_high", "same_high"):
        proj = torch.randn(B, M, 6 * E, generator=g) * 0.1
        lift = 20.0                                     # c * lift * lift = 0.25 * 400 = 100
        first = 3 * E if c["kind"] == "pair_high" else 4 * E
        proj[:, :, first:first + E:E // H] += lift      # qpair or qsame: component 0 of every head
        proj[:, :, E:2 * E:E // H] += lift              # k of every node
    else:
        proj = torch.randn(B, M, 6 * E, generator=g)
        proj[..., 0:E] = 0
        proj[..., 3 * E:] = 0
    return dict(proj=proj, dout=torch.randn(B, M, E, generator=g))


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (op, r64, r32): operands and the restatement's float64 / float32 outputs {"y", "dproj" (cases with a backward)};
    r64["_scale"]: the largest |value| per output.  Computed once; nothing may modify it."""
    c = CASES[name]
    op = operands(name)
    runs = []
    for dtype in (torch.float64, torch.float32):
        if c["bwd"]:
            y, d = ham_ref.hetero_mha_backward(op["proj"], op["dout"], H, dtype)
            runs.append(dict(y=y, dproj=d))
        else:
            with torch.no_grad():
                runs.append(dict(y=ham_ref.hetero_mha(op["proj"], H, dtype)))
    r64, r32 = runs
    r64["_scale"] = {k: float(v.abs().max()) for k, v in r64.items()}
    return op, r64, r32


def error(name, got, r64):
    """max-abs for the value y, the norm of the difference for the gradient dproj."""
    d = got.double() - r64[name]
    return float(d.abs().max()) if name == "y" else float(d.norm())


def bound(c, name, r64, r32):
    scale = max(error(name, r32[name], r64), U * r64["_scale"][name])
    return MARGIN * RATIO.get((name, c["kind"]), 1.0) * scale


def fixture_weights(fx):
    return {k: torch.from_numpy(np.ascontiguousarray(fx[k])) for k in ham_ref.WEIGHT_KEYS}
