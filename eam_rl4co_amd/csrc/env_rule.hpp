// The step-and-mask rule of every routing env, stated once: the per-node predicates and per-row transitions that the five
// walkers (the step kernels and state replay of env_reward.hip / pdp.hip, env_step_row of decode_step.hip, the finishing
// wavefront of rollout_resident.hip, the state update of rollout_multistart.hip) apply in their own loops and layouts.
// Scalars in, scalars out: no pointers, lanes or reductions here.  The order of the float operations is part of the
// numerical contract (-ffp-contract=off); tests/test_gpu_step_rule.py holds every walker to tests/step_ref.py on rows
// that sit ON each comparison.
#pragma once
#include "dmath.hpp"

namespace eamrl {
namespace rule {

// torch's norm(p=2, dim=-1) of a 2-vector on the CPU, bit for bit (OP): sqrtf(fmaf(dy, dy, dx * dx))
__device__ __forceinline__ float leg(float ax, float ay, float bx, float by)
{
    const float dx = ax - bx, dy = ay - by;
    return __builtin_sqrtf(fma_(dy, dy, dx * dx));
}

// ---- CVRPEnv._step + get_action_mask (cvrp/env.py:68-100,132-144); CVRPTW inherits them ---------------------------------
__device__ __forceinline__ float cvrp_limit(float vcap) { return vcap + 1e-5f; }      // per row, before the node loop

__device__ __forceinline__ float cvrp_load_after(float used, float dem_a, bool to_depot)
{
    return (used + dem_a) * (to_depot ? 0.0f : 1.0f);
}

// V: the walker's own visited flag (a 0/1 int or a bool), so that the `|` is the one the walker had
template <typename V>
__device__ __forceinline__ int cvrp_blocked(V visited, float dem_n, float used, float lim)
{
    return visited | ((dem_n + used) > lim);
}

// the depot is closed only while the vehicle stands on it with a customer still free (CVRP, SDVRP, CVRPTW)
__device__ __forceinline__ bool depot_open(bool at_depot, bool any_free) { return !(at_depot && any_free); }

// ---- the clock of CVRPTWEnv._step + get_action_mask (cvrptw/env.py:103-138) -------------------------------------------
__device__ __forceinline__ float tw_clock_after(float now, float leg, float win_start, float dur_a, bool to_depot)
{
    const float arrive = now + leg;
    const float start = arrive > win_start ? arrive : win_start;
    return (to_depot ? 0.0f : 1.0f) * (start + dur_a);
}

__device__ __forceinline__ bool tw_in_time(float now, float leg, float win_end) { return (now + leg) <= win_end; }

// ---- SDVRPEnv._step + get_action_mask (sdvrp/env.py:58-92,137-146): deliver min(remaining demand, free capacity) --------
__device__ __forceinline__ void sdvrp_deliver(float sel_rem, float used, float vcap, bool to_depot, float& used_out,
                                              float& left_out)
{
    const float free_cap = vcap - used;
    const float delivered = sel_rem < free_cap ? sel_rem : free_cap;
    used_out = (used + delivered) * (to_depot ? 0.0f : 1.0f);
    left_out = sel_rem + (-delivered);
}

__device__ __forceinline__ bool sdvrp_full(float used, float vcap) { return used >= vcap; }      // per row, before the node loop
__device__ __forceinline__ bool sdvrp_blocked(float rem_n, bool full) { return (rem_n == 0.0f) | full; }
__device__ __forceinline__ bool sdvrp_has_demand(float rem_n) { return rem_n > 0.0f; }      // done = no node has any

// ---- OPEnv._step + get_action_mask (op/env.py:69-102,149-165): limit_n = the latest arrival that still reaches the depot -
__device__ __forceinline__ bool op_exceeds(float tour_len, float leg, float limit_n) { return (tour_len + leg) > limit_n; }

// ---- PCTSPEnv._step + get_action_mask (pctsp/env.py:64-97,156-163) ------------------------------------------------------
__device__ __forceinline__ bool pctsp_depot_open(float prize_total, bool any_unvisited)
{
    return !((prize_total < 1.0f) && any_unvisited);
}

// OP and PCTSP end on a depot visit after the first step (op/env.py:69-102, pctsp/env.py:64-97)
template <typename I>
__device__ __forceinline__ bool tour_ends(bool to_depot, I istep) { return to_depot && istep > 0; }

// ---- PDPEnv._step (pdp/env.py:66-106): the reference's modulo -- the delivery of a pickup; for a delivery (or the depot) the
// depot or a pickup, which is open already
template <typename I>
__device__ __forceinline__ I pdp_partner(I a, int M) { return (a + (M - 1) / 2) % M; }

}  // namespace rule
}  // namespace eamrl
