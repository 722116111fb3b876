"""CPU: the encoder attention forward's dispatch (eamrl_mha_encoder_variant: host arithmetic, no launch) -- the decision table on
both sides of every edge under no debug key, key 15 and key 3, the Python restatement that labels the large-graph GPU cases
(attn_large_cases.fwd_kernel) against the library, and the launcher's source holding each condition once."""
import ctypes as C
import os
import re

import pytest

import attn_large_cases as ac
from test_host_linear import debug_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QKV, OUT = 0x10000000, 0x20000000          # never dereferenced
IDS = dict(X2=1, MFMA=2, TILED=3, PLAIN16=4, PLAIN32=5)
E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from eam_rl4co_amd import _lib

    return _lib.load()


def variant_of(lib, N, keys=(), qkv=QKV, out=OUT, B=2, E=128, H=8):
    """eamrl_mha_encoder_variant on fake pointers."""
    with debug_keys(lib, keys):
        return lib.eamrl_mha_encoder_variant(C.c_void_p(qkv), C.c_void_p(out), B, N, E, H)


def test_header_declares_the_variant_ids_and_the_entry_point():
    from eam_rl4co_amd import _lib

    with open(os.path.join(ROOT, "include", "eamrl.h")) as f:
        text = f.read()
    defines = {k: int(v) for k, v in re.findall(r"#define\s+EAMRL_MHA_(\w+)\s+(\d+)", text)}
    assert defines == IDS and len(set(defines.values())) == len(defines)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+eamrl_mha_encoder_variant\s*\(", code)
    assert len(_lib.PROTOTYPES["eamrl_mha_encoder_variant"]) == 6
    assert _lib.load().eamrl_version() == 101


# E = 128, H = 8, aligned pointers: N -> (no key, key 15, key 3)
TABLE = {1: ("X2", "X2", "PLAIN16"), 127: ("X2", "X2", "PLAIN16"), 128: ("MFMA", "TILED", "PLAIN16"),
         1200: ("MFMA", "TILED", "PLAIN16"), 1201: ("TILED", "TILED", "PLAIN16"), 1280: ("TILED", "TILED", "PLAIN16"),
         1281: ("TILED", "TILED", None)}


@pytest.mark.parametrize("N", sorted(TABLE))
def test_the_decision_table_on_both_sides_of_every_edge(lib, N):
    want = [IDS[w] if w else E_ARG for w in TABLE[N]]
    assert [variant_of(lib, N), variant_of(lib, N, keys=(15,)), variant_of(lib, N, keys=(3,))] == want
    # key 3 wins over key 15; a qkv or an out 4 bytes off a 16-byte boundary takes the key 3 column, whatever key 15 says
    assert variant_of(lib, N, keys=(3, 15)) == want[2]
    for keys in ((), (15,)):
        assert variant_of(lib, N, keys=keys, qkv=QKV + 4) == want[2]
        assert variant_of(lib, N, keys=keys, out=OUT + 4) == want[2]
    assert variant_of(lib, N, B=0) == want[0]                     # an empty batch decides like any other


def test_head_widths_and_head_counts(lib):
    for keys in ((), (15,), (3,)):
        assert variant_of(lib, 5, keys=keys, E=256) == IDS["PLAIN32"]                    # D = 32
        assert variant_of(lib, 640, keys=keys, E=256) == IDS["PLAIN32"]                  # 2 * 640 * 32 floats = 160 KiB
        assert variant_of(lib, 641, keys=keys, E=256) == E_ARG
        assert variant_of(lib, 20, keys=keys, E=64) == E_ARG                             # D = 8
        assert variant_of(lib, 20, keys=keys, H=2) == E_ARG                              # D = 64
        assert variant_of(lib, 20, keys=keys, E=96, H=6) == IDS["PLAIN16"]               # D = 16, H % 4 != 0
        assert variant_of(lib, 1281, keys=keys, E=96, H=6) == E_ARG
    # D = 16 in groups of 4 heads but not E = 128, H = 8: the MFMA kernel does not apply
    assert [variant_of(lib, N, E=64, H=4) for N in (127, 128, 1281)] == [IDS["X2"], IDS["TILED"], IDS["TILED"]]
    # B * H beyond a grid dimension; the tiled kernel's grid beyond it: the plain kernel, which takes B * H blocks
    assert variant_of(lib, 20, B=2 ** 28) == E_ARG and variant_of(lib, 20, B=2 ** 28 - 1) == IDS["X2"]
    assert variant_of(lib, 1201, B=2 ** 27) == IDS["PLAIN16"] and variant_of(lib, 1281, B=2 ** 27) == E_ARG


def test_the_entry_point_has_the_guards_of_eamrl_mha_encoder(lib):
    p, q = C.c_void_p(QKV), C.c_void_p(OUT)
    good = [p, q, 2, 20, 128, 8]
    assert lib.eamrl_mha_encoder_variant(*good) == IDS["X2"]
    for i, v in ((0, None), (1, None), (2, -1), (3, 0), (4, 0), (5, 0), (5, 3)):
        bad = list(good)
        bad[i] = v
        for fn, args in (("eamrl_mha_encoder_variant", bad), ("eamrl_mha_encoder", bad + [None])):
            assert getattr(lib, fn)(*args) == E_ARG
            assert fn.encode() + b": requirement failed" in lib.eamrl_last_error(), fn


def test_the_python_restatement_agrees_with_the_library(lib):
    """attn_large_cases.fwd_kernel labels the GPU cases of tests/test_gpu_attention_large.py; this ties it to the code."""
    for N in sorted(set(ac.ORACLE_SIZES + ac.FWD_ONLY)):
        for key15 in (False, True):
            got = variant_of(lib, N, keys=(15,) if key15 else (), B=1)
            assert got == {"mfma": IDS["MFMA"], "tiled": IDS["TILED"]}[ac.fwd_kernel(N, key15)], (N, key15)


def test_one_copy_of_the_dispatch_conditions():
    with open(os.path.join(ROOT, "eam_rl4co_amd", "csrc", "encoder.hip")) as f:
        text = f.read()
    assert text.count("g_debug[3]") == 1 and text.count("g_debug[15]") == 1
    assert text.count("160 * 1024") == 1 and text.count("mha_encoder_mfma_supports(") == 1
    launch = text[text.index("int launch_mha_encoder("):]
    launch = launch[:launch.index("\n}\n")]
    assert "mha_encoder_variant(" in launch and "uintptr_t" not in launch and "g_debug" not in launch
    # one launch per id: four kernels of this file, and the MFMA kernel's in the file that holds it
    assert launch.count("hipLaunchKernelGGL") == len(IDS) - 1 and launch.count("launch_mha_encoder_mfma(") == 1
    assert launch.count("case EAMRL_MHA_") == len(IDS)
    with open(os.path.join(ROOT, "eam_rl4co_amd", "csrc", "encoder_attn_mfma.hip")) as f:
        mfma = f.read()
    mfma = mfma[mfma.index("int launch_mha_encoder_mfma("):]
    assert mfma[:mfma.index("\n}\n")].count("hipLaunchKernelGGL") == 1
