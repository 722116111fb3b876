"""The case table of tests/test_host_rollout_call.py and tests/golden/make_golden_rollout_call.py: argument validation of the five
whole-rollout entry points (include/eamrl.h), on hand-built structs with dummy 16-byte-aligned addresses.

For each entry point and each env it accepts there is one valid call (B = 4 instances, 4 rows per instance, E = 128, H = 8; TSP
with 20 nodes, the depot envs with 21) and the calls derived from it by breaking exactly one thing.  NOTHING HERE MAY RUN WHERE A
GPU IS PRESENT: a valid call passes validation and launches on the made-up addresses (without a device the launch fails at once
with EAMRL_E_LAUNCH, which is what the valid cases record).

    cases()      -> [(id, entry, env, call dict, breaks)]     breaks: the derivation violates a requirement (EAMRL_E_ARG expected)
    invoke(c)    -> (return code, message of eamrl_last_error)
    predicates() -> {key: answer} of the four host-only shape queries over M in {1, 2, 112, 113}, S in {1, 2, 128, 129}, every env
"""
import copy
import ctypes as C

E_ARG, E_LAUNCH = -1, -2
GREEDY, SAMPLE, EVALUATE = 0, 1, 2
ENVS = {"tsp": 0, "cvrp": 1, "sdvrp": 2, "pctsp": 3, "op": 4, "cvrptw": 5, "pdp": 6}
B, S, E, H = 4, 4, 128, 8
ENTRIES = {
    "eamrl_am_rollout": tuple(ENVS),
    "eamrl_am_rollout_seeded": tuple(ENVS),
    "eamrl_am_rollout_polynet": ("tsp", "cvrp"),
    "eamrl_am_rollout_polynet_seeded": ("tsp", "cvrp"),
    "eamrl_am_rollout_eas_layer": ("tsp", "cvrp"),
}
# the eamrl_state members a fused rollout of the env reads or writes
STATE = {
    "tsp": ("cur", "mask", "done", "first", "istep"),
    "cvrp": ("cur", "mask", "done", "used", "vcap", "visited", "demand"),
    "sdvrp": ("cur", "mask", "done", "used", "vcap", "rem"),
    "pctsp": ("cur", "mask", "done", "used", "vcap", "visited", "demand", "istep"),
    "op": ("cur", "mask", "done", "used", "vcap", "visited", "demand", "istep", "locs"),
    "cvrptw": ("cur", "mask", "done", "used", "vcap", "time", "visited", "demand", "locs", "tw", "dur"),
    "pdp": ("cur", "mask", "done", "visited", "to_deliver"),
}
POLY_PTRS = ("Wout", "W1", "ctab", "W2", "b2", "L")
LAYER_PTRS = ("W1", "b1", "W2", "b2")
_next = [0x100000]


def addr():
    """A fresh made-up address, 16-byte aligned, never followed."""
    _next[0] += 0x1000
    return _next[0]


def base(entry, env):
    """One valid call of `entry` on `env`, as a dict of plain values."""
    M = 20 if env == "tsp" else 21
    cache = {n: addr() for n in ("K", "V", "Lp", "Pa", "gctx")}
    if env != "pdp":
        cache["cvec"] = addr()
    if env == "tsp":
        cache["Pb"] = addr()
    if env == "sdvrp":
        cache["dyn"] = addr()
    cache.update(ld=(6 if env == "tsp" else 5) * E, B=B, M=M, E=E, H=H)
    c = dict(entry=entry, env=ENVS[env], cache=cache, state={n: addr() for n in STATE[env]}, R=S * B, mode=GREEDY, noise=None,
             given=None, t_given=0, seeded=0, seed=1234, seed_dev=None, noise_scratch=None, clip=10.0, temp=1.0, top_k=0, top_p=0.0,
             t_max=2 * M + 1, actions=addr(), logps=addr(), steps_out=addr(), status=addr())
    if entry.endswith("_seeded"):
        c.update(mode=SAMPLE, seeded=1)
    if entry == "eamrl_am_rollout_seeded" and env == "pdp":
        c["noise_scratch"] = addr()         # no kernel with in-place noise serves PDP: the draws go through the caller's scratch
    if "polynet" in entry:
        c["poly"] = dict({n: addr() for n in POLY_PTRS}, k=4, P=256, s_offset=0)
    if "eas_layer" in entry:
        c["layer"] = dict({n: addr() for n in LAYER_PTRS}, forced=None, t_forced=0)
    return c


def _set(path, value):
    def f(c):
        d = c
        for k in path[:-1]:
            d = d[k]
        d[path[-1]] = value
    return f


def _bump(path, by=4):
    def f(c):
        d = c
        for k in path[:-1]:
            d = d[k]
        d[path[-1]] += by
    return f


def _other_env(c):
    """PCTSP with a complete PCTSP state and cache: an env the extensions are not built for."""
    o = base("eamrl_am_rollout", "pctsp")
    c.update(env=o["env"], cache=o["cache"], state=o["state"], t_max=o["t_max"])


def mutations(entry, env):
    """[(name, edit)]: each edit breaks exactly one requirement of the valid call."""
    b = base(entry, env)
    seeded_entry = entry.endswith("_seeded")
    m = [(f"cache_{n}_null", _set(("cache", n), None)) for n in ("K", "V", "Lp", "Pa", "cvec", "Pb", "dyn") if n in b["cache"]]
    m += [(f"state_{n}_null", _set(("state", n), None)) for n in STATE[env]]
    m += [(f"{n}_null", _set((n,), None)) for n in ("actions", "logps", "steps_out", "status")]
    m += [("t_max_0", _set(("t_max",), 0)), ("R_not_multiple_of_B", _set(("R",), S * B + 1)), ("temp_0", _set(("temp",), 0.0)),
          ("K_misaligned", _bump(("cache", "K")))]
    if entry == "eamrl_am_rollout":
        m.append(("top_p_1.5", _set(("top_p",), 1.5)))
    if not seeded_entry:
        m.append(("sample_without_noise_or_seed", _set(("mode",), SAMPLE)))
        m.append(("evaluate_without_given", lambda c: c.update(mode=EVALUATE, t_given=5)))
        m.append(("evaluate_t_given_0", lambda c: c.update(mode=EVALUATE, given=addr(), t_given=0)))
    if "polynet" in entry:
        m += [(f"poly_{n}_null", _set(("poly", n), None)) for n in POLY_PTRS]
        m += [(f"poly_{n}_misaligned", _bump(("poly", n))) for n in POLY_PTRS]
        m += [("poly_null", _set(("poly",), None)), ("poly_P_128", _set(("poly", "P"), 128)), ("poly_k_0", _set(("poly", "k"), 0)),
              ("poly_s_offset_negative", _set(("poly", "s_offset"), -1)),
              ("poly_s_offset_out_of_range", _set(("poly", "s_offset"), 0x7fffffff // B)),
              ("poly_heads_out_set", _set(("state", "heads_out"), addr())),
              ("rows_per_instance_1", _set(("R",), B))]
    if "eas_layer" in entry:
        m += [(f"layer_{n}_null", _set(("layer", n), None)) for n in LAYER_PTRS]
        m += [(f"layer_{n}_misaligned", _bump(("layer", n))) for n in LAYER_PTRS]
        m += [("layer_null", _set(("layer",), None)), ("layer_forced_without_t_forced", _set(("layer", "forced"), addr())),
              ("layer_heads_out_misaligned", _set(("state", "heads_out"), addr() + 4)),
              ("seeded_without_sample_mode", _set(("seeded",), 1)),
              ("rows_per_instance_1", _set(("R",), B)), ("rows_per_instance_129", _set(("R",), 129 * B))]
    if "polynet" in entry or "eas_layer" in entry:
        m += [("M_113", _set(("cache", "M"), 113)), ("env_pctsp", _other_env)]
    return m


def cases():
    out = []
    for entry, envs in ENTRIES.items():
        for env in envs:
            out.append((f"{entry}/{env}/valid", entry, env, base(entry, env), False))
            for name, edit in mutations(entry, env):
                c = copy.deepcopy(base(entry, env))
                edit(c)
                out.append((f"{entry}/{env}/{name}", entry, env, c, True))
    return out


def _struct(cls, d):
    s = cls()
    for k, v in d.items():
        setattr(s, k, v)
    return s


def invoke(c):
    """Calls the entry point of `c` -> (return code, eamrl_last_error() as str)."""
    from eam_rl4co_amd import _lib

    lib = _lib.load()
    cs, ss = _struct(_lib.Cache, c["cache"]), _struct(_lib.State, c["state"])
    head = (c["env"], C.byref(cs), C.byref(ss))
    tail = (c["clip"], c["temp"])
    outs = (c["t_max"], c["actions"], c["logps"], c["steps_out"], c["status"], None)
    entry = c["entry"]
    if "polynet" in entry:
        ps = None if c["poly"] is None else _struct(_lib.PolyNet, c["poly"])
        head += (None if ps is None else C.byref(ps),)
    if "eas_layer" in entry:
        ls = None if c["layer"] is None else _struct(_lib.EasLayer, c["layer"])
        head += (None if ls is None else C.byref(ls),)
    if entry == "eamrl_am_rollout":
        args = head + (c["R"], c["mode"], c["noise"], c["given"], c["t_given"]) + tail + (c["top_k"], c["top_p"]) + outs
    elif entry == "eamrl_am_rollout_seeded":
        args = head + (c["R"], C.c_uint64(c["seed"]), c["seed_dev"], c["noise_scratch"]) + tail + outs
    elif entry == "eamrl_am_rollout_polynet":
        args = head + (c["R"], c["mode"], c["noise"], c["given"], c["t_given"]) + tail + outs
    elif entry == "eamrl_am_rollout_polynet_seeded":
        args = head + (c["R"], C.c_uint64(c["seed"]), c["seed_dev"]) + tail + outs
    else:
        args = head + (c["R"], c["mode"], c["noise"], c["given"], c["t_given"], c["seeded"], C.c_uint64(c["seed"]), c["seed_dev"]) \
            + tail + outs
    rc = getattr(lib, entry)(*args)
    msg = lib.eamrl_last_error()
    return rc, (msg.decode() if msg else "")


def predicates():
    """The four host-only shape queries on shape-only caches (no pointer is set)."""
    from eam_rl4co_amd import _lib

    lib = _lib.load()
    out = {}
    for env, e in ENVS.items():
        for M in (1, 2, 112, 113):
            for rows in (1, 2, 128, 129):
                cs = _struct(_lib.Cache, dict(ld=(6 if env == "tsp" else 5) * E, B=B, M=M, E=E, H=H))
                R = rows * B
                key = f"{env}/M{M}/S{rows}"
                out[f"eamrl_rollout_kernel/{key}"] = lib.eamrl_rollout_kernel(e, C.byref(cs), R, 2 * M + 1, 0, 0.0)
                out[f"eamrl_rollout_rng_native/{key}"] = lib.eamrl_rollout_rng_native(e, C.byref(cs), R)
                out[f"eamrl_rollout_polynet_supported/{key}"] = lib.eamrl_rollout_polynet_supported(e, C.byref(cs), R)
                out[f"eamrl_rollout_eas_layer_supported/{key}"] = lib.eamrl_rollout_eas_layer_supported(e, C.byref(cs), R)
    return out
