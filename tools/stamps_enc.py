"""Development only: phase breakdown of the fused encoder kernel (needs tools/build_stamps.sh;
EAMRL_HIP_LIB=tools/_stamps/libeamrl_hip.so python tools/stamps_enc.py [M] [B] [bench]).

Without `bench` the kernel runs on given embeddings (h_in) and stores them, no cache.  With `bench` it runs what bench.py
runs: the init embedding inside the kernel, the decoder cache and the graph context, the embeddings never stored (so the
"load h" row is the init embedding, and the constants / graph context / cache rows are filled)."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("tests", "tests/golden"):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), p))
from eam_rl4co_amd import _lib  # noqa: E402
import eam_rl4co_amd as ea  # noqa: E402


def main():
    argv = [a for a in sys.argv[1:] if a != "bench"]
    bench = "bench" in sys.argv[1:]
    M = int(argv[0]) if len(argv) > 0 else 100
    B = int(argv[1]) if len(argv) > 1 else 1024
    lib = _lib.load()
    pol = ea.AttentionModelPolicy(env_name="tsp").eval().to("cuda")
    if bench:
        env = ea.get_env("tsp", generator_params=dict(num_loc=M), seed=1)
        torch.manual_seed(0)
        td = env.reset(batch_size=[B]).to("cuda")
        spec = pol.decoder._fused_cache_spec(B, M, "cuda")
        fused = pol.encoder.net._fused_layers(None, (M, 128))
        init = pol.encoder.init_embedding.fused_spec(td)
        init["want_init"] = False
        run = lambda: pol.encoder.net(None, None, cache_spec=spec, init=init, store_hidden=False, fused=fused)
    else:
        h = torch.randn(B, M, 128, device="cuda") * 0.5
        run = lambda: pol.encoder.net(h)
    out = (C.c_ulonglong * 24)()
    names = ["load h / init embedding", "P1 epilogue (q k v store)", "  barrier", "P2 attention", "  barrier", "P3 out_proj partial",
             "  barrier", "norm1", "P4 epilogue (relu store)", "  barrier", "P5 ffn2 partial", "  barrier", "norm2", "store h",
             "P4 prologue (b0, bias)", "P4 gemm", "P1 prologue (bias)", "P1 gemm", "constants staging + barrier", "graph context",
             None, "cache passes"]
    rows = [i for i, n in enumerate(names) if n is not None]
    for it in range(3):
        torch.cuda.synchronize()
        lib.eamrl_debug_read_enc_stamps(out, 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        with torch.no_grad():
            run()
        e1.record()
        torch.cuda.synchronize()
        lib.eamrl_debug_read_enc_stamps(out, 0)
        waves = out[20]
        tot = sum(out[i] for i in rows)
        print(f"run {it}: kernel {e0.elapsed_time(e1)*1e3:.0f} us, waves {waves}, ticks/wave {tot/waves:.0f}")
        for i in rows:
            print(f"   {names[i]:28s} {out[i]/waves:9.0f} ticks/wave  {100*out[i]/tot:5.1f} %")


if __name__ == "__main__":
    main()
