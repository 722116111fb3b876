"""No GPU needed: eamrl_rollout_kernel, the host-only query that names the kernel a whole-rollout call runs on
(include/eamrl.h).  It is the function the dispatcher of eamrl_am_rollout branches on, so these answers are the dispatch:
a top-k / top-p call goes to the register-resident kernel's filtering variant up to 112 nodes -- multistart batches
included, because the start-sharing MFMA kernel does not filter -- and to the streaming kernel above.

The cache structs are built by hand (E = 128, H = 8) with dummy row addresses: the query reads the shape fields only and
launches nothing.
"""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSP, CVRP = 0, 1
B = 8


def cache_struct(M, env="tsp", E=128, H=8, batch=B):
    from eam_rl4co_amd import _lib

    c = _lib.Cache()
    slots = 6 if env == "tsp" else 5
    for i, name in enumerate(("K", "V", "Lp", "Pa", "Pb")):
        setattr(c, name, C.c_void_p(0x10000 + 4 * E * i))       # 16-byte aligned, never followed
    c.cvec, c.gctx = C.c_void_p(0x20000), C.c_void_p(0x30000)
    c.ld, c.B, c.M, c.E, c.H = slots * E, batch, M, E, H
    return c


def test_the_query_is_declared_exported_and_bound():
    from eam_rl4co_amd import _lib, ops

    with open(os.path.join(ROOT, "include", "eamrl.h")) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+eamrl_rollout_kernel\s*\(([^)]*)\)\s*;", code)
    assert m, "eamrl_rollout_kernel is not declared in include/eamrl.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.rsplit(" ", 1)[0].replace(" ", "") for a in args] == ["int", "consteamrl_cache*", "int64_t", "int", "int", "double"]
    consts = {n: int(v) for n, v in re.findall(r"#define\s+EAMRL_KERNEL_(MS_MFMA|RESIDENT|STREAM)\s+(\d+)", code)}
    assert sorted(consts) == ["MS_MFMA", "RESIDENT", "STREAM"] and len(set(consts.values())) == 3
    assert "eamrl_rollout_kernel" in _lib.PROTOTYPES
    lib = _lib.load()          # binds every prototype; raises if the library does not export one
    assert callable(lib.eamrl_rollout_kernel)
    # the Python names are the header's constants
    assert [ops.ROLLOUT_KERNELS[consts[n]] for n in ("MS_MFMA", "RESIDENT", "STREAM")] == ["ms_mfma", "resident", "stream"]


def test_kernel_choice_on_hand_built_caches():
    from eam_rl4co_amd import ops

    c100 = cache_struct(100)
    assert ops.rollout_kernel("tsp", c100, B, 100, top_p=0.9) == "resident"
    assert ops.rollout_kernel("tsp", c100, B, 100, top_k=5) == "resident"
    assert ops.rollout_kernel("tsp", c100, B, 100, top_k=6, top_p=0.9) == "resident"
    # the filtering variant ends at 112 nodes; without a filter the resident kernel goes on to 128
    assert ops.rollout_kernel("tsp", cache_struct(112), B, 112, top_p=0.9) == "resident"
    assert ops.rollout_kernel("tsp", cache_struct(113), B, 113, top_p=0.9) == "stream"
    assert ops.rollout_kernel("tsp", cache_struct(113), B, 113, top_k=5) == "stream"
    assert ops.rollout_kernel("tsp", cache_struct(113), B, 113) == "resident"
    assert ops.rollout_kernel("tsp", cache_struct(129), B, 129) == "stream"
    # multistart: the start-sharing kernel without a filter, the resident kernel's start loop with one
    assert ops.rollout_kernel("tsp", c100, 4 * B, 100) == "ms_mfma"
    assert ops.rollout_kernel("tsp", c100, 4 * B, 100, top_k=5) == "resident"
    assert ops.rollout_kernel("tsp", c100, 4 * B, 100, top_p=0.9) == "resident"
    assert ops.rollout_kernel("tsp", cache_struct(113), 4 * B, 113, top_p=0.9) == "stream"
    # the neutral settings are "no filter"
    for R in (B, 4 * B):
        for M in (100, 113):
            c = cache_struct(M)
            plain = ops.rollout_kernel("tsp", c, R, M)
            for kw in (dict(top_p=1.0), dict(top_k=0), dict(top_k=0, top_p=1.0), dict(top_k=0, top_p=0.0)):
                assert ops.rollout_kernel("tsp", c, R, M, **kw) == plain, (R, M, kw)
    # the other envs, and an episode bound beyond what the kernel keeps in LDS
    cv = cache_struct(101, "cvrp")
    assert ops.rollout_kernel("cvrp", cv, B, 2 * 101 + 1, top_p=0.9) == "resident"
    assert ops.rollout_kernel("cvrp", cv, B, 1000, top_p=0.9) == "stream"
    # other model sizes stream
    assert ops.rollout_kernel("tsp", cache_struct(100, E=256, H=8), B, 100, top_p=0.9) == "stream"


def test_kernel_choice_follows_the_debug_switches():
    from eam_rl4co_amd import _lib, ops

    lib = _lib.load()
    c = cache_struct(100)
    try:
        assert lib.eamrl_debug_set(1, 1) == 0          # force streaming, as the GPU tests do
        assert ops.rollout_kernel("tsp", c, B, 100, top_p=0.9) == "stream"
        assert ops.rollout_kernel("tsp", c, B, 100) == "stream"
        assert ops.rollout_kernel("tsp", c, 4 * B, 100) == "ms_mfma"
    finally:
        lib.eamrl_debug_set(1, 0)
    assert ops.rollout_kernel("tsp", c, B, 100, top_p=0.9) == "resident"


def test_bad_arguments_are_rejected():
    from eam_rl4co_amd import _lib, ops

    lib = _lib.load()
    c = cache_struct(100)
    ok = lambda *a: lib.eamrl_rollout_kernel(TSP, C.byref(c), *a)
    assert ok(B, 100, 0, 0.0) >= 0
    assert ok(B, 100, 0, 1.5) < 0 and b"eamrl_rollout_kernel" in lib.eamrl_last_error()        # top_p > 1
    assert ok(B + 1, 100, 0, 0.9) < 0                                                           # R % B != 0
    assert ok(B, 100, -1, 0.0) < 0 and ok(B, 100, 0, -0.1) < 0
    assert ok(0, 100, 0, 0.0) < 0 and ok(B, 0, 0, 0.0) < 0
    assert lib.eamrl_rollout_kernel(TSP, None, B, 100, 0, 0.0) < 0
    assert lib.eamrl_rollout_kernel(17, C.byref(c), B, 100, 0, 0.0) < 0
    with pytest.raises(RuntimeError, match="eamrl_rollout_kernel"):
        ops.rollout_kernel("tsp", c, B + 1, 100, top_p=0.9)
    with pytest.raises(RuntimeError, match="eamrl_rollout_kernel"):
        ops.rollout_kernel("tsp", c, B, 100, top_p=1.5)
