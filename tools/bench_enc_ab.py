"""Two builds of the library timed alternately in ONE process on the fp32 fused encoder (A/B yardstick for kernel changes).

    bash tools/build_variant.sh parent           # in a checkout of the parent commit; copy the library over
    python tools/bench_enc_ab.py --a tools/_variants/parent/libeamrl_hip.so --b eam_rl4co_amd/lib/libeamrl_hip.so \
        [--rounds 7] [--iters 20] [--batch 1024] [--nodes 100] [--json out.json]

Rows: the encoder launch alone (AM: 3 layers, batch norm, init embedding + cache tail + graph context; POMO: 6 layers, instance
norm) at TSP-`nodes` x `batch`.  Every round times each build once (`iters` launches between two events), in alternating
order; reported per build: mean, min, max and standard deviation over the rounds, and the outputs of the two builds are
compared bit for bit.  Both libraries live in the process at once; the binding's handle is switched between them.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), p) for p in ("", "tests", "tests/golden")]

import eam_rl4co_amd as ea  # noqa: E402
from eam_rl4co_amd import _lib  # noqa: E402
from bench_enc16 import make_policy, timed  # noqa: E402


def load_lib(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, argtypes in _lib.PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = _lib._RESTYPES.get(name, C.c_int)
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True)
    ap.add_argument("--b", required=True)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    _lib.load()
    libs = {"a": load_lib(args.a), "b": load_lib(args.b)}
    env = ea.get_env("tsp", generator_params=dict(num_loc=args.nodes), seed=1)
    torch.manual_seed(0)
    td = env.reset(batch_size=[args.batch]).to(dev)
    B, M = td["action_mask"].shape
    rows = {}
    for cfg, what in (("am_tsp", "encoder_am"), ("pomo_tsp", "encoder_pomo")):
        pol = make_policy(cfg, dev)
        pol.precision = "32-true"
        spec = pol.decoder._fused_cache_spec(B, M, dev, dtype=pol._dtype16)
        if not pol.decoder.use_graph_context:
            spec.pop("Wg", None), spec.pop("gctx", None)
        fused = pol.encoder.net._fused_layers(None, (M, 128))
        init = pol.encoder.init_embedding.fused_spec(td)
        init["want_init"] = False

        def fn():
            return pol.encoder.net(None, None, cache_spec=spec, init=init, store_hidden=False, fused=fused)

        samples, outs = {"a": [], "b": []}, {}
        with torch.no_grad():
            for k in ("a", "b"):
                _lib._lib = libs[k]
                timed(fn, args.iters)    # warm-up: kernel attributes, clocks
                outs[k] = spec["buf"].clone()
            for r in range(args.rounds):
                for k in (("a", "b") if r % 2 == 0 else ("b", "a")):
                    _lib._lib = libs[k]
                    samples[k].append(timed(fn, args.iters))
        row = {"bit_identical": bool(torch.equal(outs["a"].view(torch.int32), outs["b"].view(torch.int32)))}
        for k, v in samples.items():
            row[k] = {"mean_ms": round(statistics.mean(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                      "stdev_ms": round(statistics.stdev(v), 4) if len(v) > 1 else 0.0, "rounds_ms": [round(x, 4) for x in v]}
        row["b_over_a"] = round(row["b"]["mean_ms"] / row["a"]["mean_ms"], 4)
        rows[what] = row
        print(json.dumps({what: row}), flush=True)
    out = {"workload": f"tsp{M} x {B}", "a": args.a, "b": args.b, "iters": args.iters, "rows": rows}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
