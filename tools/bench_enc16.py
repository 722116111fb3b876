"""fp32 vs bf16 vs fp16 fused encoder, timed alternately in one process (AttentionModelPolicy(precision=...)).

    python tools/bench_enc16.py [--iters 20] [--batch 1024] [--json out.json]

Rows: the encoder kernel alone at TSP-100 (AM: 3 layers, batch norm, init embedding + cache tail + graph context) and at
POMO TSP-100 (6 layers, instance norm, no graph context), and the whole greedy `policy(td, env, phase="test")` at TSP-100.
Every round times each precision once, in rotating order; the median over rounds is reported.  Under
`rocprofv3 --kernel-trace --stats` the same run gives the per-kernel times (k_encoder_fused vs k_encoder_fused16<T, 7>).
"""
import argparse
import json
import os
import sys

import torch

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), p) for p in ("", "tests", "tests/golden")]

import eam_rl4co_amd as ea  # noqa: E402
from _util import golden_weights  # noqa: E402

PRECISIONS = ("32-true", "bf16-mixed", "16-mixed")
PEAK16_TFLOPS = 2500.0       # MI355X dense fp16 / bf16 MFMA (spec)


def make_policy(cfg, dev):
    kw = dict(num_encoder_layers=6, normalization="instance", use_graph_context=False) if cfg.startswith("pomo") else {}
    pol = ea.AttentionModelPolicy(env_name="tsp", **kw).eval()
    sd = pol.state_dict()
    for k, v in golden_weights(cfg).items():
        sd[k].copy_(torch.from_numpy(v))
    return pol.to(dev)


def encoder_flops(M, layers, cache_slots):
    """Algorithmic FLOPs of one instance: the Linears, QK^T and WV of every layer, the cache projections."""
    E, F = 128, 512
    lin = 2 * M * E * (3 * E + E + F) + 2 * M * F * E
    att = 2 * 2 * M * M * E
    return layers * (lin + att) + 2 * M * E * E * cache_slots


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    env = ea.get_env("tsp", generator_params=dict(num_loc=100), seed=1)
    torch.manual_seed(0)
    td = env.reset(batch_size=[args.batch]).to(dev)
    B, M = td["action_mask"].shape
    rows = {}
    for cfg, what in (("am_tsp", "encoder_am"), ("pomo_tsp", "encoder_pomo"), ("am_tsp", "rollout_greedy")):
        pol = make_policy(cfg, dev)
        spec_fn = pol.encoder.init_embedding.fused_spec
        nl = len(pol.encoder.net.layers)

        def run(prec):
            pol.precision = prec
            if what == "rollout_greedy":
                return lambda: pol(td, env, phase="test", decode_type="greedy")
            spec = pol.decoder._fused_cache_spec(B, M, dev, dtype=pol._dtype16)
            if not pol.decoder.use_graph_context:
                spec.pop("Wg", None), spec.pop("gctx", None)
            fused = pol.encoder.net._fused_layers(None, (M, 128))
            init = spec_fn(td)
            init["want_init"] = False
            return lambda: pol.encoder.net(None, None, cache_spec=spec, init=init, store_hidden=False, fused=fused)

        fns = {}
        with torch.no_grad():
            for p in PRECISIONS:
                fns[p] = run(p)
                fns[p]()                 # warm-up: packs, kernel attributes
            torch.cuda.synchronize()
            samples = {p: [] for p in PRECISIONS}
            for r in range(args.rounds):
                order = PRECISIONS[r % 3:] + PRECISIONS[:r % 3]
                for p in order:
                    pol.precision = p
                    samples[p].append(timed(fns[p], args.iters))
        pol.precision = "32-true"
        med = {p: sorted(v)[len(v) // 2] for p, v in samples.items()}
        row = {p: round(med[p], 4) for p in PRECISIONS}
        row.update({f"ratio_{p}": round(med[p] / med["32-true"], 3) for p in PRECISIONS[1:]})
        if what != "rollout_greedy":
            fl = B * encoder_flops(M, nl, 6)
            row.update({f"tflops_{p}": round(fl / (med[p] * 1e-3) / 1e12, 1) for p in PRECISIONS})
            row.update({f"frac_peak16_{p}": round(fl / (med[p] * 1e-3) / 1e12 / PEAK16_TFLOPS, 3) for p in PRECISIONS[1:]})
        rows[what] = row
        print(json.dumps({what: row}), flush=True)
    out = {"workload": f"tsp100 x {B}", "unit": "ms (median of rounds)", "rows": rows}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
