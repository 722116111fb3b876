#!/usr/bin/env python3
"""Generate the EAS-Lay golden vectors under tests/golden/ by RUNNING THE REFERENCE.

    python tests/golden/make_golden_eas_lay.py

Same machinery as make_golden_polynet.py: reference modules through `_refshim`, and an empty stub package for
`rl4co.models.zoo.eas`, whose `__init__` imports the Lightning search module.  Only `zoo/eas/nn.py` (EASLayerNet) and
`zoo/eas/decoder.py` (forward_pointer_attn_eas_lay) are loaded, next to the reference's own PointerAttention.

Writes eas_lay_pointer.npz: the inputs of one pointer call with the layer in place (N = 3 instances, 6 queries each, M = 20
nodes, E = 128, 8 heads; non-zero W2 and b2), the raw logits the reference returns, and autograd's gradients of the four layer
parameters for the fixed linear functional sum(C * logits).  Data only.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refshim  # noqa: E402,F401
import make_golden  # noqa: E402,F401  (installs the shim's packages)

import torch  # noqa: E402

import rl4co.models.zoo.am.policy as ref_am_policy  # noqa: E402

_zoo = os.path.dirname(os.path.dirname(ref_am_policy.__file__))
if "rl4co.models.zoo.eas" not in sys.modules:
    _stub = types.ModuleType("rl4co.models.zoo.eas")
    _stub.__path__ = [os.path.join(_zoo, "eas")]
    sys.modules["rl4co.models.zoo.eas"] = _stub

from rl4co.models.nn.attention import PointerAttention  # noqa: E402
from rl4co.models.zoo.eas.decoder import forward_pointer_attn_eas_lay  # noqa: E402
from rl4co.models.zoo.eas.nn import EASLayerNet  # noqa: E402

N, Q, M, E, H = 3, 6, 20, 128, 8


def main():
    g = torch.Generator().manual_seed(20221)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    ptr = PointerAttention(E, H, mask_inner=True, out_bias=False, check_nan=True)
    with torch.no_grad():
        ptr.project_out.weight.copy_(rn(E, E, scale=E ** -0.5))
    layer = EASLayerNet(N, E)
    with torch.no_grad():
        layer.W1.copy_(rn(N, E, E, scale=0.1))
        layer.b1.copy_(rn(N, 1, E, scale=0.3))
        layer.W2.copy_(rn(N, E, E, scale=0.08))
        layer.b2.copy_(rn(N, 1, E, scale=0.1))
    ptr.eas_layer = layer
    ptr.forward = types.MethodType(forward_pointer_attn_eas_lay, ptr)
    query, key, value, logit_key = rn(N, Q, E), rn(N, M, E), rn(N, M, E), rn(N, M, E, scale=2.0)
    mask = torch.rand(N, Q, M, generator=g) < 0.6
    mask[..., 0] = True                     # no query without a feasible node
    C = rn(N, Q, M)
    logits = ptr(query, key, value, logit_key, mask)
    assert logits.shape == (N, Q, M)
    grads = torch.autograd.grad((C * logits).sum(), [layer.W1, layer.b1, layer.W2, layer.b2])
    np_ = lambda t: t.detach().numpy()
    fx = dict(query=np_(query), key=np_(key), value=np_(value), logit_key=np_(logit_key), mask=np_(mask), C=np_(C),
              Wout=np_(ptr.project_out.weight), W1=np_(layer.W1), b1=np_(layer.b1), W2=np_(layer.W2), b2=np_(layer.b2),
              logits=np_(logits), dW1=np_(grads[0]), db1=np_(grads[1]), dW2=np_(grads[2]), db2=np_(grads[3]))
    path = os.path.join(HERE, "eas_lay_pointer.npz")
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    assert size <= 1 << 20, f"{size} bytes is above the committed-file limit"
    print(f"eas_lay_pointer.npz {size} bytes; max|logit| {float(logits.detach().abs().max()):.3f}")


if __name__ == "__main__":
    main()
