"""The attention forward kernels of two builds of the library, timed alternately in ONE process (the yardstick of a refactor that
moved their code): the parent commit's build loaded twice (P1, P2: the parent against itself is the spread of the measurement)
and the tree's (T).

    python tools/time_attn_ab.py --parent-lib DIR/libeamrl_hip.so --parent-lib-copy DIR/copy_of_it.so \
        [--tree-lib eam_rl4co_amd/lib/libeamrl_hip.so] [--rounds 5] [--out profiles/rNNx_attn_ab.json]

(The copy is a second file with the same bytes, so that the loader maps it separately.)  Cases, at the sizes the project quotes:
  k_mha_encoder_mfma   512 x 501                       k_mha_encoder_x2   1024 x 100
  k_mha_encoder_tiled  1 x 1281, 512 x 501 (key 15)    k_hetero_mha       1024 x 101, 1024 x 129
Per case and round: 3 warm-up launches per build, then 20 launches per build, one at a time in rotating order P1, P2, T, each
between two HIP events; the figure of a build in a round is the median of its 20.  Over the rounds: reference = the median of
P1's figures, spread = the largest |P2 - P1| of a round, tree = the median of T's figures; within_margin: tree <= reference +
spread.  The outputs of the parent and of the tree are compared bit for bit.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eam_rl4co_amd import _lib, ops  # noqa: E402

SLOTS = ("P1", "P2", "T")


def load_lib(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, argtypes in _lib.PROTOTYPES.items():
        if hasattr(lib, name):              # the parent lacks what the tree adds
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = _lib._RESTYPES.get(name, C.c_int)
    return lib


def one_launch_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--parent-lib-copy", required=True)
    ap.add_argument("--tree-lib", default=os.path.join(ROOT, "eam_rl4co_amd", "lib", "libeamrl_hip.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU timing"
    assert os.path.realpath(args.parent_lib) != os.path.realpath(args.parent_lib_copy)
    _lib.load()
    libs = dict(P1=load_lib(args.parent_lib), P2=load_lib(args.parent_lib_copy), T=load_lib(args.tree_lib))
    torch.manual_seed(11)
    cases = [("k_mha_encoder_mfma 512x501", "mha", 512, 501, ()), ("k_mha_encoder_x2 1024x100", "mha", 1024, 100, ()),
             ("k_mha_encoder_tiled 1x1281", "mha", 1, 1281, ()), ("k_mha_encoder_tiled 512x501 key15", "mha", 512, 501, (15,)),
             ("k_hetero_mha 1024x101", "hetero", 1024, 101, ()), ("k_hetero_mha 1024x129", "hetero", 1024, 129, ())]
    rows = {}
    for name, what, B, N, keys in cases:
        x = torch.randn(B, N, (3 if what == "mha" else 6) * 128, device="cuda")
        fn = (lambda: ops.mha_encoder(x, 8)) if what == "mha" else (lambda: ops.hetero_mha(x, 8))
        for lib in libs.values():
            for k in keys:
                assert lib.eamrl_debug_set(k, 1) == 0
        try:
            outs, figs = {}, {s: [] for s in SLOTS}
            for s in SLOTS:
                _lib._lib = libs[s]
                for _ in range(3):
                    outs[s] = fn()
            torch.cuda.synchronize()
            for r in range(args.rounds):
                t = {s: [] for s in SLOTS}
                for i in range(20):
                    for j in range(3):
                        s = SLOTS[(i + j + r) % 3]
                        _lib._lib = libs[s]
                        t[s].append(one_launch_ms(fn))
                for s in SLOTS:
                    figs[s].append(statistics.median(t[s]))
        finally:
            for lib in libs.values():
                for k in keys:
                    lib.eamrl_debug_set(k, 0)
        ref, tree = statistics.median(figs["P1"]), statistics.median(figs["T"])
        spread = max(abs(a - b) for a, b in zip(figs["P1"], figs["P2"]))
        row = {"rounds_ms": {s: [round(v, 5) for v in figs[s]] for s in SLOTS}, "parent_ms": round(ref, 5), "tree_ms": round(tree, 5),
               "parent_spread_ms": round(spread, 5), "tree_over_parent": round(tree / ref, 4),
               "within_margin": bool(tree <= ref + spread),
               "bit_identical": bool(torch.equal(outs["P1"].view(torch.int32), outs["T"].view(torch.int32)))}
        rows[name] = row
        print(json.dumps({name: row}), flush=True)
    _lib._lib = libs["T"]
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "launches_per_round_and_build": 20, "warmups": 3, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
