"""HAM against AM on pickup and delivery, and the heterogeneous attention kernel against the plain one, on the same build in
one process, timed alternately.

    python tools/time_ham_vs_am.py [--batch 1024] [--num-loc 100] [--rounds 5] [--reps 10] [--json out.json]

whole    `policy(td, env, phase="test", decode_type="greedy")`: encoder + cache + decode loop + reward (env.reset excluded), host
         clock around a device synchronise.  Three policies: HAM, AM as it runs by default (up to 112 nodes: the fused
         all-layers encoder, one launch), AM layer by layer (EAMRL_FUSED_ENCODER=0: the same launch structure as HAM's encoder).
encoder  `policy.encoder(td)` alone, HIP events.
kernel   `ops.hetero_mha` on proj [B, M, 6E] against `ops.mha_encoder` on its q | k | v third, HIP events, at M = num_loc + 1 and
         at M = 129 (both on fp32 MFMA there); with the useful operations of each (score and value products, 2 flops per
         multiply-add) over the kernel time.
parts    the HAM layer's stages at M = num_loc + 1: projections (three GEMMs, one gather, one scatter), attention kernel, W_out
         GEMM with residual and norm, FFN.
Every round takes the median over `reps` calls of each variant in turn; the median over the rounds is reported together with
the rounds themselves (their spread is the run-to-run noise a ratio has to be read against).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import eam_rl4co_amd as ea  # noqa: E402
from eam_rl4co_amd import ops  # noqa: E402

DEV = "cuda"
E, H, D = 128, 8, 16


def events(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(variants, rounds, reps, timer):
    """{name: fn} -> {name: {"ms": median over rounds, "rounds": [...]}}; every round visits the variants in turn."""
    for fn in variants.values():
        for _ in range(5):
            fn()
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            res[k].append(statistics.median(timer(fn) for _ in range(reps)))
    return {k: {"ms": round(statistics.median(v), 4), "rounds": [round(x, 4) for x in v]} for k, v in res.items()}


def attention_flops(B, M, hetero):
    """Multiply-adds the formula needs, times 2: general scores and value products M x M x D per head; hetero adds one extra
    score per non-depot (row, key) pair and the pair term."""
    P = (M - 1) // 2
    mac = 2 * M * M * D
    if hetero:
        mac += (2 * P) * (2 * P) * D + 2 * (2 * P) * D
    return 2.0 * mac * H * B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--num-loc", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU timing"
    B, N = args.batch, args.num_loc
    torch.manual_seed(7)
    env = ea.get_env("pdp", generator_params=dict(num_loc=N), seed=7)
    td = env.reset(batch_size=[B]).to(DEV)
    ham = ea.HeterogeneousAttentionModelPolicy().eval().to(DEV)
    am = ea.AttentionModelPolicy(env_name="pdp").eval().to(DEV)

    def unfused(fn):
        def run():
            os.environ["EAMRL_FUSED_ENCODER"] = "0"
            try:
                return fn()
            finally:
                del os.environ["EAMRL_FUSED_ENCODER"]
        return run

    out = {"what": f"greedy rollout, {B} instances x PDP-{N}, one MI355X, fp32, untrained policies, eager policy calls; "
                   f"{args.rounds} rounds (variants alternating) of the median over {args.reps} calls"}
    with torch.no_grad():
        call = lambda pol: (lambda: pol(td, env, phase="test", decode_type="greedy"))
        out["whole_ms"] = alternate({"ham": call(ham), "am": call(am), "am_layer_by_layer": unfused(call(am))},
                                    args.rounds, args.reps, host)
        enc = lambda pol: (lambda: pol.encoder(td))
        out["encoder_ms"] = alternate({"ham": enc(ham), "am": enc(am), "am_layer_by_layer": unfused(enc(am))},
                                      args.rounds, args.reps, events)
        out["kernel"] = {}
        for M in sorted({N + 1, 129}):
            proj = torch.randn(B, M, 6 * E, device=DEV)
            qkv = proj[..., :3 * E].contiguous()
            r = alternate({"hetero_mha": lambda: ops.hetero_mha(proj, H), "mha_encoder": lambda: ops.mha_encoder(qkv, H)},
                          args.rounds, args.reps, events)
            for k, hetero in (("hetero_mha", True), ("mha_encoder", False)):
                r[k]["useful_tflops"] = round(attention_flops(B, M, hetero) / (r[k]["ms"] * 1e-3) / 1e12, 2)
            r["hetero_over_plain"] = round(r["hetero_mha"]["ms"] / r["mha_encoder"]["ms"], 3)
            r["useful_flops_ratio"] = round(attention_flops(B, M, True) / attention_flops(B, M, False), 3)
            out["kernel"][f"M{M}"] = r
        layer = ham.encoder.layers[0]
        mha, ffn = layer[0].module, layer[2].module
        h = ham.encoder.init_embedding(td)
        proj = mha.project(h)
        att = ops.hetero_mha(proj, H)
        bn1, bn2 = layer[1].fused_bn(), layer[3].fused_bn()
        h1 = ops.linear(att, mha.packed()["out"], None, residual=h, bn=bn1)

        def ffn_():
            x = ops.linear(h1, ffn[0].weight, ffn[0].bias, relu=True)
            return ops.linear(x, ffn[2].weight, ffn[2].bias, residual=h1, bn=bn2)

        out["ham_layer_parts_ms"] = alternate({
            "project": lambda: mha.project(h), "hetero_mha": lambda: ops.hetero_mha(proj, H),
            "out_gemm_norm": lambda: ops.linear(att, mha.packed()["out"], None, residual=h, bn=bn1), "ffn": ffn_,
            "whole_layer": lambda: layer(h)}, args.rounds, args.reps, events)
    w, e = out["whole_ms"], out["encoder_ms"]
    out["ham_over_am_whole"] = round(w["ham"]["ms"] / w["am"]["ms"], 3)
    out["ham_over_am_layer_by_layer_whole"] = round(w["ham"]["ms"] / w["am_layer_by_layer"]["ms"], 3)
    out["ham_over_am_encoder"] = round(e["ham"]["ms"] / e["am"]["ms"], 3)
    out["ham_over_am_layer_by_layer_encoder"] = round(e["ham"]["ms"] / e["am_layer_by_layer"]["ms"], 3)
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
