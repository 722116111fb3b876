"""GPU: the device-memory path of the evolutionary improvement (eamrl_ea_tsp_run_large / eamrl_ea_cvrp_run_large, csrc/
evolution_large.hip) -- populations and graphs of up to 1024 -- held to what the LDS kernel is held to in test_gpu_next.py:
the reference's recorded runs, oracle/ea_oracle.py on the same draws (identical tours, bit-equal fitness), and the LDS
kernel itself bit for bit where both serve a shape."""
import numpy as np
import pytest
import torch

from _util import golden
from test_gpu_next import _cvrp_oracle_run, _oracle_ea
from test_gpu_parity import DEV, assert_bits_equal, make_policy, t

pytestmark = pytest.mark.gpu


def _tsp_golden_run(g, kernel):
    import eam_rl4co_amd as ea

    env = ea.get_env("tsp", generator_params=dict(num_loc=g["locs"].shape[1]))
    td = ea.TensorDict({"locs": t(g["locs"])}, batch_size=[g["locs"].shape[0]])
    runner = ea.EA(env, dict(num_generations=int(g["num_generations"]), mutation_rate=float(g["mutation_rate"]),
                             crossover_rate=float(g["crossover_rate"]), selection_rate=float(g["selection_rate"])))
    d = ea.EADraws(t(g["cross_rand"]), t(g["cross_idx"]), t(g["mut_rand"]), t(g["mut_idx"]))
    init = t(g["init_pop"])
    pop, fit = runner.run(init, td, draws=d, kernel=kernel)
    assert torch.equal(init, t(g["init_pop"]))                                  # input untouched
    return pop, fit, d


def _cvrp_golden_run(g, kernel):
    import eam_rl4co_amd as ea

    B, M = g["locs"].shape[:2]
    env = ea.get_env("cvrp", generator_params=dict(num_loc=M - 1))
    td = ea.TensorDict({"locs": t(g["locs"]), "demand": t(g["demand"]),
                        "vehicle_capacity": torch.full((B, 1), float(g["vehicle_capacity"]), device=DEV)}, batch_size=[B])
    runner = ea.EA(env, dict(num_generations=int(g["num_generations"]), mutation_rate=float(g["mutation_rate"]),
                             crossover_rate=float(g["crossover_rate"]), selection_rate=float(g["selection_rate"]),
                             method="am" if int(g["top_k"]) else None))
    d = ea.EACvrpDraws(t(g["init_mut_rand"]), t(g["init_mut_u"]), t(g["cross_rand"]), t(g["cross_u"]), t(g["mut_rand"]),
                       t(g["mut_u"]))
    pop, fit = runner.run(t(g["init_pop"]), td, draws=d, kernel=kernel)
    return pop, fit, d


# ---- 1. the committed reference runs on the large path, and against the LDS kernel ---------------------------------------
@pytest.mark.parametrize("name", ["ea_tsp20_default", "ea_tsp20_busy", "ea_tsp50_busy", "ea_cvrp20_default", "ea_cvrp20_busy",
                                  "ea_cvrp50_am"])
def test_large_path_reproduces_reference_run_and_the_lds_kernel(name):
    g = golden(name)
    run = _tsp_golden_run if "tsp" in name else _cvrp_golden_run
    pop, fit, _ = run(g, "large")
    np.testing.assert_array_equal(pop.cpu().numpy(), g["pop"])                  # the reference's evolved tours
    np.testing.assert_allclose(fit.cpu().numpy(), g["fitness"], rtol=1e-5, atol=1e-5)
    lpop, lfit, _ = run(g, "lds")
    assert torch.equal(pop, lpop)
    assert_bits_equal(fit, lfit.cpu().numpy(), "fitness, large against lds")


# ---- 2. TSP against the oracle beyond the LDS kernel's limits ----------------------------------------------------------------
BOTH = [(0.1, 0.6, 0.2), (0.9, 1.0, 1.0)]
TSP_CASES = [(N, S, B, G, dup, r) for (N, S, B, G, dup) in [(129, 8, 2, 2, False), (128, 129, 2, 2, True), (130, 130, 2, 2, False),
                                                            (192, 64, 2, 2, True), (200, 40, 3, 3, False)] for r in BOTH]
TSP_CASES += [(1024, 4, 1, 1, False, (0.9, 1.0, 1.0)), (140, 1024, 1, 1, True, (0.5, 0.8, 0.05))]


@pytest.mark.parametrize("N,S,B,G,dup,rates", TSP_CASES)
def test_large_tsp_matches_oracle_on_random_populations(N, S, B, G, dup, rates):
    """First N and first S past the old limits (third 64-bit word of the node set; S > N forces top-k replacement), the
    multistart layout S = N, N a multiple of 64 (lane-tree block edge), the longest row with the set's last bit, the largest
    population: identical populations, bit-equal fitness, permutations, start nodes in place, per-start elitism."""
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import ops

    mr, cr, sr = rates
    assert ops.ea_kernel("tsp", S, N) == "large"
    rng = np.random.default_rng(N * 1000 + S)
    locs = rng.random((B, N, 2), dtype=np.float32)
    init = np.zeros((B, S, N), dtype=np.int64)
    for b in range(B):
        for s in range(S):
            first = ((s // 2) if dup else s) % N
            rest = rng.permutation(N - 1)
            init[b, s] = np.concatenate([[first], rest + (rest >= first)])
    if S > N:
        dup = True
    env = ea.get_env("tsp", generator_params=dict(num_loc=N))
    td = ea.TensorDict({"locs": t(locs)}, batch_size=[B])
    runner = ea.EA(env, dict(num_generations=G, mutation_rate=mr, crossover_rate=cr, selection_rate=sr))
    gen = torch.Generator(device=DEV).manual_seed(N + S)
    d = ea.EADraws.sample(G, B, S, N, sr, DEV, gen)
    pop, fit = runner.run(t(init), td, draws=d)
    opop, ofit = _oracle_ea(locs, init, G, mr, float(np.float32(cr)), sr, d)
    np.testing.assert_array_equal(pop.cpu().numpy(), opop)
    assert_bits_equal(fit, ofit, "fitness")
    p = pop.cpu().numpy()
    assert (np.sort(p, axis=-1) == np.arange(N)).all()                          # still permutations
    if not dup:
        np.testing.assert_array_equal(p[:, :, 0], init[:, :, 0])                # start nodes stay in place
        f0 = runner.get_fitness(t(init), td).cpu().numpy()
        assert (fit.cpu().numpy() >= f0).all()                                  # elitist per start node


# ---- 3. CVRP against the oracle on rollout populations -------------------------------------------------------------------
@pytest.mark.parametrize("N,S", [(128, 8), (127, 129), (130, 130), (200, 40)])
@pytest.mark.parametrize("top_k", [False, True])
@pytest.mark.parametrize("rates", BOTH)
def test_large_cvrp_matches_oracle_on_rollout_populations(N, S, top_k, rates):
    """Populations = sampled rollouts of the untrained policy: min(S, N) multistart rows, the rest (S > N) from a second
    sampled rollout, so first nodes repeat there.  The rows are handed over at the full length a CVRP rollout may have,
    env_spec.max_steps = 2 M + 1 > 256 entries, zero-padded as evolution_worker hands action rows over.  Identical tours,
    bit-equal fitness, feasible results; method="am" (top-k) and the default replacement."""
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import env_spec, ops

    B, G = 2, 2
    mr, cr, sr = rates
    env = ea.get_env("cvrp", generator_params=dict(num_loc=N), seed=N)
    torch.manual_seed(N + S)
    td = env.reset(batch_size=[B]).to(DEV)
    pol = make_policy("am_cvrp")
    L = env_spec.max_steps("cvrp", N + 1)
    assert L == 2 * (N + 1) + 1 and L > 256 and ops.ea_kernel("cvrp", S, N, L) == "large"
    parts, left = [], S
    while left > 0:
        s = min(left, N)
        with torch.no_grad():
            out = pol(td.clone(), env, phase="train", decode_type="multistart_sampling", num_starts=s)
        rows = ea.unbatchify(out["actions"], s)                                                  # [B, s, T]
        parts.append(torch.nn.functional.pad(rows, (0, L - rows.shape[-1])))
        left -= s
    init = torch.cat(parts, 1).contiguous()
    assert init.shape == (B, S, L)
    runner = ea.EA(env, dict(num_generations=G, mutation_rate=mr, crossover_rate=cr, selection_rate=sr,
                             method="am" if top_k else None))
    gen = torch.Generator(device=DEV).manual_seed(N * 7 + S)
    d = ea.EACvrpDraws.sample(G, B, S, sr, DEV, gen)
    pop, fit = runner.run(init, td, draws=d)
    opop, ofit = _cvrp_oracle_run(td["locs"].cpu().numpy(), td["demand"].cpu().numpy(), 1.0, init.cpu().numpy(), G, mr, cr, sr,
                                  d, top_k)
    np.testing.assert_array_equal(pop.cpu().numpy(), opop)
    assert_bits_equal(fit, ofit, "fitness")
    rows = pop.permute(1, 0, 2).reshape(-1, L)
    env.check_solution_validity(ea.batchify(td, S), rows)                       # feasible CVRP tours


# ---- 4. the reference's own runs at shapes beyond the LDS kernel ---------------------------------------------------------
@pytest.mark.parametrize("name", ["ea_large_tsp130_busy", "ea_large_cvrp129_busy", "ea_large_cvrp129_am"])
def test_large_path_reproduces_reference_run_at_new_shapes(name):
    """tests/golden/make_golden_ea_large.py: TSP-130 and CVRP with 129 customers (both replacement modes), 12 tours, 3
    generations, the reference's recorded draws."""
    from eam_rl4co_amd import ops

    g = golden(name)
    tsp = "tsp" in name
    B, S, L = g["init_pop"].shape
    assert ops.ea_kernel("tsp" if tsp else "cvrp", S, g["locs"].shape[1] - (0 if tsp else 1), L) == "large"
    pop, fit, d = (_tsp_golden_run if tsp else _cvrp_golden_run)(g, None)
    np.testing.assert_array_equal(pop.cpu().numpy(), g["pop"])                  # the reference's evolved tours
    np.testing.assert_allclose(fit.cpu().numpy(), g["fitness"], rtol=1e-5, atol=1e-5)
    G, mr, cr, sr = int(g["num_generations"]), float(g["mutation_rate"]), float(g["crossover_rate"]), float(g["selection_rate"])
    if tsp:
        _, ofit = _oracle_ea(g["locs"], g["init_pop"], G, mr, float(np.float32(cr)), sr, d)
    else:
        _, ofit = _cvrp_oracle_run(g["locs"], g["demand"], float(g["vehicle_capacity"]), g["init_pop"], G, mr, cr, sr, d,
                                   bool(g["top_k"]))
    assert_bits_equal(fit, ofit, "fitness")


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
def test_eam_step_on_tsp130_multistart():
    """TSP-130 with the reference's default num_starts = N: evolution_worker's layouts and the whole EAM step."""
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import train

    B, N = 2, 130
    env = ea.get_env("tsp", generator_params=dict(num_loc=N), seed=3)
    torch.manual_seed(3)
    td = env.reset(batch_size=[B]).to(DEV)
    pol = make_policy("pomo_tsp")
    runner = ea.EA(env, dict(num_generations=3, mutation_rate=0.3, crossover_rate=0.8, selection_rate=0.6))
    with torch.no_grad():
        out = pol(td.clone(), env, phase="train", decode_type="multistart_sampling", num_starts=N)
    gen = torch.Generator(device=DEV).manual_seed(1)
    new_actions, _, pop = ea.evolution_worker(out["actions"], td, runner, env, return_population=True, generator=gen)
    assert new_actions.shape == (N * B, N - 1) and pop.shape == (B, N, N)
    full = torch.cat([out["actions"][:, :1], new_actions], 1)
    assert (full.sort(1).values == torch.arange(N, device=DEV)).all()
    r_new = env.get_reward(ea.batchify(td, N), full)
    assert (r_new >= out["reward"] - 1e-6).all() and (r_new > out["reward"] + 1e-6).any()

    gen = torch.Generator(device=DEV).manual_seed(5)
    res = train.eam_loss(pol, env, td.clone(), runner, num_starts=N, generator=gen)
    assert torch.isfinite(res["loss"])
    assert (res["improved_reward"] >= res["reward"] - 1e-6).all()               # every row: improved >= sampled
    res["loss"].backward()
    grads = [p.grad for p in pol.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads) and sum(float(x.abs().sum()) for x in grads) > 0
    env.check_solution_validity(ea.batchify(td, N), res["improved_actions"])


def test_eam_step_on_cvrp130_single_start():
    """CVRP-130, one sampled tour per instance, a population of 50 copies, method="am" (top-k)."""
    import eam_rl4co_amd as ea

    B, N = 2, 130
    env = ea.get_env("cvrp", generator_params=dict(num_loc=N), seed=4)
    torch.manual_seed(4)
    td = env.reset(batch_size=[B]).to(DEV)
    pol = make_policy("am_cvrp")
    runner = ea.EA(env, dict(num_generations=3, mutation_rate=0.3, crossover_rate=0.8, selection_rate=0.6, method="am"))
    with torch.no_grad():
        out = pol(td.clone(), env, phase="train", decode_type="sampling")
    gen = torch.Generator(device=DEV).manual_seed(9)
    improved, _, pop = ea.evolution_worker(out["actions"], td, runner, env, return_population=True, generator=gen)
    assert improved.shape == out["actions"].shape and pop.shape == (B, 50, out["actions"].shape[1])
    env.check_solution_validity(td, improved)

    gen = torch.Generator(device=DEV).manual_seed(9)
    res = ea.eam_am_loss(pol, env, td.clone(), runner, "no", generator=gen)
    assert torch.isfinite(res["loss"]) and res["improved_actions"].shape == res["actions"].shape
    res["loss"].backward()
    grads = [p.grad for p in pol.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads) and sum(float(x.abs().sum()) for x in grads) > 0
    env.check_solution_validity(td, res["improved_actions"])
