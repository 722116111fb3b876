"""CPU (no GPU needed): the host side of the device-memory EA path -- which kernel serves a shape (eamrl_ea_kernel, the
function the dispatcher branches on), what the new entry points reject before any launch, the scratch size, and the
ValueError the Python wrappers raise beyond the limits."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSP, CVRP, PCTSP, OP = 0, 1, 3, 4
LDS, LARGE = 0, 1


def lib():
    from eam_rl4co_amd import _lib

    return _lib.load()


def test_new_entry_points_are_declared_and_bound():
    from eam_rl4co_amd import _lib, ops

    with open(os.path.join(ROOT, "include", "eamrl.h")) as f:
        code = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+eamrl_ea_kernel\s*\(\s*int\s+env\s*,\s*int\s+S\s*,\s*int\s+N\s*,\s*int\s+L\s*\)\s*;", code)
    assert re.search(r"\bsize_t\s+eamrl_ea_large_scratch_bytes\s*\(", code)
    consts = {n: int(v) for n, v in re.findall(r"#define\s+EAMRL_EA_KERNEL_(LDS|LARGE)\s+(\d+)", code)}
    assert consts == {"LDS": LDS, "LARGE": LARGE} and ops.EA_KERNELS == ("lds", "large")
    for name, extra in (("eamrl_ea_tsp_run", "eamrl_ea_tsp_run_large"), ("eamrl_ea_cvrp_run", "eamrl_ea_cvrp_run_large")):
        # the arguments of the existing entry point, then scratch and its size, then the stream
        assert _lib.PROTOTYPES[extra] == _lib.PROTOTYPES[name][:-1] + [C.c_void_p, C.c_size_t, C.c_void_p]
        m_old = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        m_new = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % extra, code)
        norm = lambda s: [" ".join(a.split()) for a in s.split(",")]
        assert norm(m_new.group(1)) == norm(m_old.group(1))[:-1] + ["void* scratch", "size_t scratch_bytes", "void* stream"]


def test_ea_kernel_names_the_path_of_a_shape():
    k = lib().eamrl_ea_kernel
    # the LDS kernel exactly where it accepts the shape today
    assert k(TSP, 128, 128, 128) == LDS and k(TSP, 100, 100, 100) == LDS and k(TSP, 1, 2, 2) == LDS
    assert k(CVRP, 93, 127, 256) == LDS and k(CVRP, 128, 127, 187) == LDS
    # one past each bound
    assert k(TSP, 129, 128, 128) == LARGE and k(TSP, 128, 129, 129) == LARGE
    assert k(CVRP, 129, 100, 100) == LARGE         # S
    assert k(CVRP, 50, 128, 200) == LARGE          # N
    assert k(CVRP, 50, 127, 257) == LARGE          # L
    assert k(CVRP, 3, 127, 258) < 0                # L beyond 2 (N + 1) + 1 serves nobody
    # the large path's own limits
    assert k(TSP, 1024, 1024, 1024) == LARGE and k(CVRP, 1024, 1023, 2049) == LARGE
    for bad in ((TSP, 1025, 200, 200), (TSP, 200, 1025, 1025), (TSP, 0, 20, 20), (TSP, 20, 1, 1), (CVRP, 1025, 200, 300),
                (CVRP, 200, 1024, 300), (CVRP, 200, 200, 404), (CVRP, 200, 200, 1)):
        assert k(*bad) == -1 and b"eamrl_ea_kernel" in lib().eamrl_last_error(), bad
    assert b"1024" in lib().eamrl_last_error()
    # PCTSP and OP keep their one kernel and its limits
    assert k(PCTSP, 128, 127, 128) == LDS and k(OP, 128, 127, 128) == LDS
    assert k(PCTSP, 129, 127, 128) == -1 and k(OP, 50, 128, 128) == -1 and k(OP, 50, 100, 129) == -1
    assert k(2, 20, 20, 20) == -1 and k(17, 20, 20, 20) == -1


def test_ea_kernel_at_the_lds_population_bound():
    """S * L <= 24000 is the LDS kernel's fourth bound.  24001 is prime, so no shape inside the other three bounds has that
    product; the bound is probed with every product from 24000 down to 23990 and up to 24010 that such a shape can have (the
    first one past the bound is 24003 = 127 * 189)."""
    k = lib().eamrl_ea_kernel
    shapes = lambda n: [(s, n // s) for s in range(1, 129) if n % s == 0 and 2 <= n // s <= 256]
    assert shapes(24001) == [] and shapes(24002) == [] and (127, 189) in shapes(24003)
    seen_lds = seen_large = 0
    for n in range(23990, 24011):
        for S, L in shapes(n):
            want = LDS if n <= 24000 else LARGE
            assert k(CVRP, S, 127, L) == want, (S, L)
            seen_lds += want == LDS; seen_large += want == LARGE
    assert seen_lds >= 2 and seen_large >= 2
    assert k(CVRP, 96, 127, 250) == LDS and k(CVRP, 127, 127, 189) == LARGE


def test_scratch_bytes_is_positive_and_monotone():
    f = lib().eamrl_ea_large_scratch_bytes
    base = f(TSP, 2, 130, 130, 0.2)
    assert base >= 3 * 2 * 130 * 130 * 2
    for env in (TSP, CVRP):
        prev = 0
        for B in (1, 2, 3, 16, 64):
            cur = f(env, B, 200, 300, 0.2); assert cur > 0 and cur >= prev; prev = cur
        prev = 0
        for S in (1, 2, 3, 128, 129, 500, 1024):
            cur = f(env, 4, S, 300, 0.2); assert cur > 0 and cur >= prev; prev = cur
        prev = 0
        for L in (2, 3, 128, 129, 1024, 2049):
            cur = f(env, 4, 200, L, 0.2); assert cur > 0 and cur >= prev; prev = cur
        prev = 0
        for rate in (0.0, 0.001, 0.01, 0.2, 0.5, 1.0, 2.0):
            cur = f(env, 4, 200, 300, rate); assert cur > 0 and cur >= prev; prev = cur
    assert f(PCTSP, 4, 20, 20, 0.2) == 0 and b"eamrl_ea_large_scratch_bytes" in lib().eamrl_last_error()
    assert f(TSP, 4, 1025, 20, 0.2) == 0 and f(TSP, 4, 20, 2050, 0.2) == 0 and f(TSP, -1, 20, 20, 0.2) == 0
    assert f(TSP, 4, 20, 20, float("nan")) == 0


def test_large_entry_points_reject_before_any_launch():
    L_ = lib()
    need = L_.eamrl_ea_large_scratch_bytes(TSP, 2, 200, 200, 0.5)
    buf = torch.zeros(need + 64, dtype=torch.uint8)           # host memory: nothing below may reach a launch
    p = buf.data_ptr() + (-buf.data_ptr()) % 16
    x = C.c_void_p(p)

    def tsp(locs=x, pop=x, fit=x, B=2, S=200, N=200, G=1, draws=x, scratch=x, nbytes=need):
        return L_.eamrl_ea_tsp_run_large(locs, pop, fit, B, S, N, G, 0.1, 0.6, 0.5, draws, draws, draws, draws, scratch, nbytes,
                                         None)

    for kw in (dict(locs=None), dict(pop=None), dict(fit=None), dict(draws=None), dict(scratch=None), dict(nbytes=need - 1),
               dict(nbytes=0), dict(N=1025), dict(S=1025), dict(N=1), dict(S=0), dict(B=-1), dict(G=-1),
               dict(scratch=C.c_void_p(p + 2))):
        assert tsp(**kw) == -1 and b"eamrl_ea_tsp_run_large" in L_.eamrl_last_error(), kw
    assert tsp(N=1025) == -1 and b"limited to 1024" in L_.eamrl_last_error()
    assert tsp(B=0) == 0                                       # an empty batch is accepted and launches nothing

    need = L_.eamrl_ea_large_scratch_bytes(CVRP, 2, 200, 403, 0.5)
    buf2 = torch.zeros(need + 64, dtype=torch.uint8)
    q = buf2.data_ptr() + (-buf2.data_ptr()) % 16
    y = C.c_void_p(q)

    def cvrp(locs=y, dem=y, vcap=y, pop=y, fit=y, B=2, S=200, N=200, L=403, G=1, init=y, draws=y, scratch=y, nbytes=need):
        return L_.eamrl_ea_cvrp_run_large(locs, dem, vcap, pop, fit, B, S, N, L, G, 0.1, 0.6, 0.5, 0, init, init, draws, draws,
                                          draws, draws, scratch, nbytes, None)

    for kw in (dict(locs=None), dict(dem=None), dict(vcap=None), dict(pop=None), dict(fit=None), dict(init=None),
               dict(draws=None), dict(scratch=None), dict(nbytes=need - 1), dict(N=1024), dict(S=1025), dict(L=404),
               dict(L=1), dict(N=0), dict(B=-1)):
        assert cvrp(**kw) == -1 and b"eamrl_ea_cvrp_run_large" in L_.eamrl_last_error(), kw
    assert cvrp(B=0) == 0
    # the existing entry points keep their limits
    assert L_.eamrl_ea_tsp_run(x, x, x, 2, 129, 100, 1, 0.1, 0.6, 0.5, x, x, x, x, None) == -1
    assert b"limited to 128" in L_.eamrl_last_error()
    assert L_.eamrl_ea_cvrp_run(y, y, y, y, y, 2, 94, 127, 256, 1, 0.1, 0.6, 0.5, 0, y, y, y, y, y, y, None) == -1
    assert b"S * L <= 24000" in L_.eamrl_last_error()


def test_wrappers_raise_value_errors_that_name_the_limit():
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import ops

    assert ops.ea_kernel("tsp", 100, 100) == "lds" and ops.ea_kernel("tsp", 130, 130) == "large"
    assert ops.ea_kernel("tsp", 20, 20, kernel="large") == "large" and ops.ea_kernel("cvrp", 20, 20, 41, kernel="lds") == "lds"
    assert ops.ea_kernel("cvrp", 100, 500, 1003) == "large" and ops.ea_kernel("pctsp", 50, 100, 101) == "lds"
    with pytest.raises(ValueError, match="1024"):
        ops.ea_kernel("tsp", 100, 1025)
    with pytest.raises(ValueError, match="1023"):
        ops.ea_kernel("cvrp", 100, 1024, 2000)
    with pytest.raises(ValueError, match="128"):
        ops.ea_kernel("op", 129, 100, 101)
    with pytest.raises(ValueError, match="LDS kernel"):
        ops.ea_kernel("tsp", 130, 130, kernel="lds")
    with pytest.raises(ValueError, match="tsp and cvrp"):
        ops.ea_kernel("pctsp", 20, 20, 21, kernel="large")
    with pytest.raises(ValueError, match="'lds' or 'large'"):
        ops.ea_kernel("tsp", 20, 20, kernel="hbm")
    # the wrappers ask before they touch a tensor's memory, so host tensors are enough to see the refusal
    B, S, N = 1, 4, 1025
    locs, pop = torch.rand(B, N, 2), torch.arange(N).repeat(B, S, 1)
    with pytest.raises(ValueError, match="1024"):
        ops.ea_tsp_run_(locs, pop, 1, 0.1, 0.6, 1.0, None, None, None, None)
    with pytest.raises(ValueError, match="1024"):
        ops.ea_cvrp_run_(torch.rand(1, 51, 2), torch.rand(1, 50), torch.ones(1), torch.zeros(1, 1025, 60, dtype=torch.int64), 1,
                         0.1, 0.6, 1.0, False, None, None, None, None, None, None)
    env = ea.get_env("op", generator_params=dict(num_loc=20))
    runner = ea.EA(env, dict(num_generations=1, mutation_rate=0.1, crossover_rate=0.6, selection_rate=0.5))
    with pytest.raises(ValueError, match="LDS kernel only"):
        runner.run(torch.zeros(1, 4, 21, dtype=torch.int64), {}, kernel="large")
