// Stand-alone environment transitions, reward and validity kernels (integer / byte work, HBM-bound).
//
//   k_tsp_step         TSPEnv._step                        rl4co/envs/routing/tsp/env.py:62-88
//   k_cvrp_step_mask   CVRPEnv._step + get_action_mask     rl4co/envs/routing/cvrp/env.py:68-100,132-144
//   k_sdvrp_step_mask  SDVRPEnv._step + get_action_mask    rl4co/envs/routing/sdvrp/env.py:58-92,137-146
//   k_pctsp_step_mask  PCTSPEnv._step + get_action_mask    rl4co/envs/routing/pctsp/env.py:64-97,156-163
//   k_tour_length      get_reward (+ PCTSP penalties)                               rl4co/utils/ops.py:59-95, tsp/env.py:152-159, cvrp/env.py:146-155
//   k_sum_logp         get_log_likelihood                  rl4co/utils/decoding.py:38-64
//   k_check_*          check_solution_validity             tsp/env.py:161-168, cvrp/env.py:157-185
//
// One 64-lane wavefront per row: the row's mask / visited bytes are read as one coalesced run, the
// "any / all" reductions are wave ballots, and the tour length uses the canonical lane tree.
// The step, mask and replay kernels walk the rows in this layout; the comparisons and transitions they apply (capacity
// epsilon, window, prize, arrival limit, split delivery, end of a tour, the leg) are the functions of env_rule.hpp.
// What a wavefront computes about a row lives in tour_row.hpp, once each: the row it owns (wave_row), the chunked lane-tree
// sum, the closed tour length, the seen-bitmap (SeenBits), the in-order log-prob sum and the CVRP load replay, and the launch
// (launch_rows).  The reward and k_check_* kernels are thin bodies over those; the k_check_* kernels restate
// check_solution_validity, whose own rules and tolerances stay here.
#include "tour_row.hpp"

namespace eamrl {

__global__ __launch_bounds__(EB) void k_tsp_step(uint8_t* mask, int64_t* first, int64_t* cur, int64_t* istep,
                                                 const int64_t* action, uint8_t* done, int64_t R, int N)
{
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    const int64_t a = action[r];
    uint8_t* m = mask + r * N;
    int any = 0;
    for (int n = lane; n < N; n += 64) {
        uint8_t v = m[n];
        if (n == a) { v = 0; m[n] = 0; }
        any |= v;
    }
    const bool remaining = __ballot(any != 0) != 0ull;
    if (lane == 0) {
        if (istep[r] == 0) first[r] = a;
        cur[r] = a;
        istep[r] += 1;
        done[r] = remaining ? 0 : 1;
    }
}

// STEP = 0: mask only (get_action_mask); STEP = 1: transition then mask
template <int STEP>
__device__ __forceinline__ void cvrp_step_mask_row(uint8_t* visited, float* used, const float* vcap,
                                                       const float* demand, int64_t* cur, uint8_t* mask, uint8_t* done, int N, int64_t rs, int64_t bi, int lane, int64_t act)
{
    const int M = N + 1;
    const float* dem = demand + bi * N;
    uint8_t* vis = visited + rs * M;
    float u = used[rs];
    int64_t c = cur[rs];
    int64_t a = -1;
    if (STEP) {
        a = act;
        int64_t di = a - 1;
        di = di < 0 ? 0 : (di > N - 1 ? N - 1 : di);
        u = rule::cvrp_load_after(u, dem[di], a == 0);
        c = a;
    }
    const float lim = rule::cvrp_limit(vcap[rs]);
    int any_free = 0;
    int all_vis = 1;
    for (int j = lane; j < N; j += 64) {
        int v = vis[j + 1] != 0;
        if (STEP && j + 1 == a) { v = 1; vis[j + 1] = 1; }
        const int blocked = rule::cvrp_blocked(v, dem[j], u, lim);
        mask[rs * M + 1 + j] = !blocked;
        any_free |= !blocked;
        all_vis &= v;
    }
    const bool any = __ballot(any_free != 0) != 0ull;
    const bool allc = __ballot(all_vis == 0) == 0ull;
    if (lane == 0) {
        int v0 = vis[0] != 0;
        if (STEP && a == 0) { v0 = 1; vis[0] = 1; }
        mask[rs * M] = rule::depot_open(c == 0, any);
        if (STEP) {
            used[rs] = u;
            cur[rs] = c;
            done[rs] = (allc && v0) ? 1 : 0;
        }
    }
}

template <int STEP>
__global__ __launch_bounds__(EB) void k_cvrp_step_mask(uint8_t* visited, float* used, const float* vcap,
                                                       const float* demand, int64_t* cur, const int64_t* action,
                                                       uint8_t* mask, uint8_t* done, int64_t R, int64_t B, int N)
{
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    cvrp_step_mask_row<STEP>(visited, used, vcap, demand, cur, mask, done, N, r, r % B, lane, STEP ? action[r] : (int64_t)-1);
}

// SDVRP: rem = demand_with_depot.  STEP = 0: mask only; STEP = 1: deliver min(rem[action], free capacity), then mask.
template <int STEP>
__global__ __launch_bounds__(EB) void k_sdvrp_step_mask(float* rem, float* used, const float* vcap, int64_t* cur,
                                                        const int64_t* action, uint8_t* mask, uint8_t* done, int64_t R,
                                                        int M)
{
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    float* rr = rem + r * M;
    float u = used[r];
    const float cap = vcap[r];
    int64_t c = cur[r];
    int64_t a = -1;
    float left = 0.0f;
    if (STEP) {
        a = action[r];
        a = a < 0 ? 0 : (a > M - 1 ? M - 1 : a);     // an out-of-range action must not become an out-of-bounds access
        rule::sdvrp_deliver(rr[a], u, cap, a == 0, u, left);
        c = a;
    }
    const bool full = rule::sdvrp_full(u, cap);
    int any_free = 0, any_rem = 0;
    for (int n = lane; n < M; n += 64) {
        float rv = rr[n];
        if (STEP && n == a) { rv = left; rr[n] = left; }
        any_rem |= rule::sdvrp_has_demand(rv);
        if (n >= 1) {
            const int blocked = rule::sdvrp_blocked(rv, full);
            mask[r * M + n] = !blocked;
            any_free |= !blocked;
        }
    }
    const bool anyf = __ballot(any_free != 0) != 0ull;
    const bool anyr = __ballot(any_rem != 0) != 0ull;
    if (lane == 0) {
        mask[r * M] = rule::depot_open(c == 0, anyf);
        if (STEP) {
            used[r] = u;
            cur[r] = c;
            done[r] = anyr ? 0 : 1;
        }
    }
}

// SDVRPEnv.check_solution_validity (sdvrp/env.py:148-171): replay the deliveries over the vector
// (-vehicle_capacity, demand...).  One wavefront per row, the vector in LDS; the replay is sequential by definition.
__global__ __launch_bounds__(EB) void k_check_sdvrp(const int64_t* actions, const float* demand, const float* vcap,
                                                    int64_t R, int64_t B, int N, int T, int32_t* bad)
{
    extern __shared__ float dem_all[];
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    const int M = N + 1;
    float* d = dem_all + (size_t)wv * M;
    const float cap = vcap[r];
    const float* dem = demand + (r % B) * N;
    for (int n = lane; n < M; n += 64) d[n] = n == 0 ? -cap : dem[n - 1];
    __builtin_amdgcn_wave_barrier();
    const int64_t* act = actions + r * T;
    float usedc = 0.0f;
    int64_t prev = -1;
    int twice = 0, range = 0;
    for (int t = 0; t < T; ++t) {
        const int64_t a = act[t];
        if (a < 0 || a > N) { range = 1; break; }
        if (t > 0 && prev == 0 && a == 0) {           // "Cannot visit depot twice if any nonzero demand"
            int nz = 0;
            for (int n = lane; n < M; n += 64) nz |= d[n] != 0.0f;
            if (__ballot(nz != 0) != 0ull) twice = 1;
        }
        const float da = d[a];
        const float free_cap = cap - usedc;
        const float dl = da < free_cap ? da : free_cap;
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) d[a] = da - dl;
        __builtin_amdgcn_wave_barrier();
        usedc = usedc + dl;
        if (a == 0) usedc = 0.0f;
        prev = a;
    }
    int nz = 0;
    for (int n = lane; n < M; n += 64) nz |= d[n] != 0.0f;
    const bool left = __ballot(nz != 0) != 0ull;
    if (lane != 0) return;
    if (range || left) atomicAdd(&bad[0], 1);
    if (twice) atomicAdd(&bad[1], 1);
}

// OP: one wavefront per row.  STEP = 0: mask only; STEP = 1: move (tour length += leg), mark visited, then mask.
template <int STEP>
__device__ __forceinline__ void op_step_mask_row(uint8_t* visited, float* tour_len, float* prize_tot, const float* prize,
                                                     const float* locs, const float* maxlen, int64_t* cur, int64_t* istep,
                                                     uint8_t* mask, uint8_t* done, int M, int64_t rs, int64_t bi, int lane, int64_t act)
{
    const float* L = locs + bi * (int64_t)M * 2;
    const float* ml = maxlen + bi * (int64_t)M;
    uint8_t* vis = visited + rs * M;
    float tl = tour_len[rs];
    int64_t c = cur[rs];
    c = c < 0 ? 0 : (c > M - 1 ? M - 1 : c);
    int64_t a = -1;
    int v0 = vis[0] != 0;
    if (STEP) {
        a = act;
        a = a < 0 ? 0 : (a > M - 1 ? M - 1 : a);     // an out-of-range action must not become an out-of-bounds access
        tl = tl + rule::leg(L[2 * a], L[2 * a + 1], L[2 * c], L[2 * c + 1]);
        c = a;
        if (a == 0) v0 = 1;
    }
    const float cx = L[2 * c], cy = L[2 * c + 1];
    for (int n = 1 + lane; n < M; n += 64) {
        int v = vis[n] != 0;
        if (STEP && n == a) { v = 1; vis[n] = 1; }
        const int over = rule::op_exceeds(tl, rule::leg(L[2 * n], L[2 * n + 1], cx, cy), ml[n]);
        mask[rs * M + n] = !(v | v0 | over);
    }
    if (lane == 0) {
        mask[rs * M] = 1;                             // the depot can always be visited
        if (STEP) {
            if (a == 0) vis[0] = 1;
            tour_len[rs] = tl;
            if (prize_tot) prize_tot[rs] = prize_tot[rs] + prize[bi * M + a];
            const int64_t i = istep[rs];
            done[rs] = rule::tour_ends(a == 0, i) ? 1 : 0;
            cur[rs] = a;
            istep[rs] = i + 1;
        }
    }
}

template <int STEP>
__global__ __launch_bounds__(EB) void k_op_step_mask(uint8_t* visited, float* tour_len, float* prize_tot, const float* prize,
                                                     const float* locs, const float* maxlen, int64_t* cur, int64_t* istep,
                                                     const int64_t* action, uint8_t* mask, uint8_t* done, int64_t R,
                                                     int64_t B, int M)
{
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    op_step_mask_row<STEP>(visited, tour_len, prize_tot, prize, locs, maxlen, cur, istep, mask, done, M, r, r % B, lane, STEP ? action[r] : (int64_t)-1);
}

// CVRPTW: CVRP transition and mask plus the clock (cvrptw/env.py:103-138).  One wavefront per row.
template <int STEP>
__device__ __forceinline__ void cvrptw_step_mask_row(uint8_t* visited, float* used, const float* vcap,
                                                         const float* demand, int64_t* cur, float* time, const float* locs,
                                                         const float* tw, const float* dur, uint8_t* mask, uint8_t* done, int N, int64_t rs, int64_t bi, int lane, int64_t act)
{
    const int M = N + 1;
    const float* dem = demand + bi * N;
    const float* L = locs + bi * (int64_t)M * 2;
    const float* W = tw + bi * (int64_t)M * 2;
    uint8_t* vis = visited + rs * M;
    float u = used[rs], now = time[rs];
    int64_t c = cur[rs];
    c = c < 0 ? 0 : (c > M - 1 ? M - 1 : c);
    int64_t a = -1;
    if (STEP) {
        a = act;
        a = a < 0 ? 0 : (a > M - 1 ? M - 1 : a);     // an out-of-range action must not become an out-of-bounds access
        now = rule::tw_clock_after(now, rule::leg(L[2 * c], L[2 * c + 1], L[2 * a], L[2 * a + 1]), W[2 * a],
                                   dur[bi * (int64_t)M + a], a == 0);
        int64_t di = a - 1;
        di = di < 0 ? 0 : (di > N - 1 ? N - 1 : di);
        u = rule::cvrp_load_after(u, dem[di], a == 0);
        c = a;
    }
    const float cx = L[2 * c], cy = L[2 * c + 1];
    const float lim = rule::cvrp_limit(vcap[rs]);
    int any_free = 0, all_vis = 1;
    for (int j = lane; j < N; j += 64) {
        int v = vis[j + 1] != 0;
        if (STEP && j + 1 == a) { v = 1; vis[j + 1] = 1; }
        const int blocked = rule::cvrp_blocked(v, dem[j], u, lim);
        const int in_time = rule::tw_in_time(now, rule::leg(cx, cy, L[2 * (j + 1)], L[2 * (j + 1) + 1]), W[2 * (j + 1) + 1]);
        mask[rs * M + 1 + j] = (!blocked) & in_time;
        any_free |= !blocked;                        // the depot rule looks at the CVRP mask only
        all_vis &= v;
    }
    const bool any = __ballot(any_free != 0) != 0ull;
    const bool allc = __ballot(all_vis == 0) == 0ull;
    if (lane == 0) {
        int v0 = vis[0] != 0;
        if (STEP && a == 0) { v0 = 1; vis[0] = 1; }
        const int in_time0 = rule::tw_in_time(now, rule::leg(cx, cy, L[0], L[1]), W[1]);
        mask[rs * M] = rule::depot_open(c == 0, any) & in_time0;
        if (STEP) {
            used[rs] = u;
            time[rs] = now;
            cur[rs] = c;
            done[rs] = (allc && v0) ? 1 : 0;
        }
    }
}

template <int STEP>
__global__ __launch_bounds__(EB) void k_cvrptw_step_mask(uint8_t* visited, float* used, const float* vcap,
                                                         const float* demand, int64_t* cur, float* time, const float* locs,
                                                         const float* tw, const float* dur, const int64_t* action,
                                                         uint8_t* mask, uint8_t* done, int64_t R, int64_t B, int N)
{
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    cvrptw_step_mask_row<STEP>(visited, used, vcap, demand, cur, time, locs, tw, dur, mask, done, N, r, r % B, lane, STEP ? action[r] : (int64_t)-1);
}

// the time-window replay of CVRPTWEnv.check_solution_validity (cvrptw/env.py:203-227): sequential, one thread per row
__global__ void k_check_cvrptw_time(const int64_t* actions, const float* locs, const float* tw, const float* dur, int64_t R,
                                    int64_t B, int M, int T, int32_t* bad)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const float* L = locs + (r % B) * (int64_t)M * 2;
    const float* W = tw + (r % B) * (int64_t)M * 2;
    float curr = 0.0f;
    int64_t node = 0;
    int late = 0;
    for (int t = 0; t < T; ++t) {
        const int64_t nx = actions[r * T + t];
        if (nx < 0 || nx >= M) { late = 1; break; }
        int ct = (int)(curr + rule::leg(L[2 * node], L[2 * node + 1], L[2 * nx], L[2 * nx + 1]));
        const int ws = (int)W[2 * nx];
        ct = ws > ct ? ws : ct;
        if ((float)ct > W[2 * nx + 1]) late = 1;
        curr = (float)ct + dur[(r % B) * (int64_t)M + nx];
        node = nx;
        if (nx == 0) curr = 0.0f;
    }
    if (late) atomicAdd(&bad[0], 1);
}

// OPEnv._get_reward: lane tree over the steps of prize[a_t]
__global__ __launch_bounds__(EB) void k_op_reward(const float* prize, const int64_t* actions, float* reward, int64_t R,
                                                  int64_t B, int M, int T)
{
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    const float* pz = prize + (r % B) * (int64_t)M;
    const int64_t* act = actions + r * T;
    const float total = chunked_tree_sum(T, lane, [&](int t) { return pz[clamp_node(act[t], M)]; });
    if (lane == 0) reward[r] = total;
}

// OPEnv.check_solution_validity (op/env.py:179-212): one wavefront per row
__global__ __launch_bounds__(EB) void k_check_op(const int64_t* actions, const float* locs, const float* maxlen, int64_t R,
                                                 int64_t B, int M, int T, int32_t* bad)
{
    __shared__ uint32_t seen_all[ROWS_PER_BLOCK][128];
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    const SeenBits seen{seen_all[wv]};
    seen.clear(128, lane);
    const int64_t* act = actions + r * T;
    const float* L = locs + (r % B) * (int64_t)M * 2;
    int bad_lane = 0;
    // the closed length over the actions, marking each step's node on the way: a customer twice is invalid, the depot may repeat
    const float length = chunked_tree_sum(T, lane, [&](int t) {
        int64_t a0 = act[t], a1 = act[(t + 1 == T) ? 0 : t + 1];      // both loads before the mark
        if (a0 < 0 || a0 >= M) { bad_lane = 1; a0 = 0; }
        else if (a0 != 0 && seen.mark(a0)) bad_lane = 1;
        a1 = clamp_node(a1, M);
        return rule::leg(L[2 * a1], L[2 * a1 + 1], L[2 * a0], L[2 * a0 + 1]);
    });
    const bool invalid = __ballot(bad_lane != 0) != 0ull;
    int ex = 0;
    const float* ml = maxlen + (r % B) * (int64_t)M;
    for (int n = lane; n < M; n += 64) {
        const float lim = ((ml[n] + rule::leg(L[0], L[1], L[2 * n], L[2 * n + 1])) + 1e-6f) + 1e-5f;
        ex |= !(length <= lim);
    }
    const bool over = __ballot(ex != 0) != 0ull;
    if (lane != 0) return;
    if (invalid) { atomicAdd(&bad[0], 1); return; }
    if (over) atomicAdd(&bad[1], 1);
}

// PCTSP: one wavefront per row.  STEP = 0: mask only; STEP = 1: collect prize (and penalty), mark visited, then mask.
// prize / penalty [B][M] with a zero depot slot; pen_tot / penalty may be null together.
template <int STEP>
__device__ __forceinline__ void pctsp_step_mask_row(uint8_t* visited, float* prize_tot, float* pen_tot,
                                                        const float* prize, const float* penalty, int64_t* cur,
                                                        int64_t* istep, uint8_t* mask,
                                                        uint8_t* done, int M, int64_t rs, int64_t bi, int lane, int64_t act)
{
    uint8_t* vis = visited + rs * M;
    float pt = prize_tot[rs];
    int64_t a = -1;
    int v0 = vis[0] != 0;
    if (STEP) {
        a = act;
        a = a < 0 ? 0 : (a > M - 1 ? M - 1 : a);     // an out-of-range action must not become an out-of-bounds access
        pt = pt + prize[bi * M + a];
        if (a == 0) v0 = 1;
    }
    int unvisited = 0;
    for (int n = 1 + lane; n < M; n += 64) {
        int v = vis[n] != 0;
        if (STEP && n == a) { v = 1; vis[n] = 1; }
        mask[rs * M + n] = !(v | v0);
        unvisited |= !v;
    }
    const bool unv = __ballot(unvisited != 0) != 0ull;
    if (lane == 0) {
        mask[rs * M] = rule::pctsp_depot_open(pt, unv);
        if (STEP) {
            if (a == 0) vis[0] = 1;
            prize_tot[rs] = pt;
            if (pen_tot) pen_tot[rs] = pen_tot[rs] + penalty[bi * M + a];
            const int64_t i = istep[rs];
            done[rs] = rule::tour_ends(a == 0, i) ? 1 : 0;
            cur[rs] = a;
            istep[rs] = i + 1;
        }
    }
}

template <int STEP>
__global__ __launch_bounds__(EB) void k_pctsp_step_mask(uint8_t* visited, float* prize_tot, float* pen_tot,
                                                        const float* prize, const float* penalty, int64_t* cur,
                                                        int64_t* istep, const int64_t* action, uint8_t* mask,
                                                        uint8_t* done, int64_t R, int64_t B, int M)
{
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    pctsp_step_mask_row<STEP>(visited, prize_tot, pen_tot, prize, penalty, cur, istep, mask, done, M, r, r % B, lane, STEP ? action[r] : (int64_t)-1);
}

// PCTSPEnv.check_solution_validity (pctsp/env.py:189-205): one wavefront per row.  bad[0] += rows with a customer
// visited twice (or an id out of range), bad[1] += rows that neither collect a prize >= 1 - 1e-5 nor visit everyone.
__global__ __launch_bounds__(EB) void k_check_pctsp(const int64_t* actions, const float* prize, int64_t R, int64_t B, int M,
                                                    int T, int32_t* bad)
{
    __shared__ uint32_t seen_all[ROWS_PER_BLOCK][128];
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    const SeenBits seen{seen_all[wv]};
    seen.clear(128, lane);
    const int64_t* act = actions + r * T;
    int bad_lane = 0, cnt = 0;      // cnt: distinct customers
    for (int t = lane; t < T; t += 64) {
        const int64_t a = act[t];
        if (a < 0 || a >= M) { bad_lane = 1; continue; }
        if (a == 0) continue;
        if (seen.mark(a)) bad_lane = 1;
        else ++cnt;
    }
    const bool invalid = __ballot(bad_lane != 0) != 0ull;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane != 0) return;
    if (invalid) { atomicAdd(&bad[0], 1); return; }
    const float* pz = prize + (r % B) * M;
    float p = 0.0f;
    for (int t = 0; t < T; ++t) p = p + pz[act[t]];
    if (!((p >= (float)(1.0 - 1e-5)) || cnt == M - 1)) atomicAdd(&bad[1], 1);
}

// penalty != null (PCTSP, with_depot): reward = saved penalties - (length + all penalties), pctsp/env.py:165-187;
// the penalty sums go through the same lane tree as the legs.
__global__ __launch_bounds__(EB) void k_tour_length(const float* locs, const int64_t* actions, float* reward, int64_t R,
                                                    int64_t B, int M, int T, int with_depot, const float* penalty)
{
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    const float* L = locs + (r % B) * (int64_t)M * 2;
    const int64_t* act = actions + r * T;
    const float total = closed_tour_length(L, act, T, M, with_depot != 0, lane);
    if (penalty) {
        const float* pen = penalty + (r % B) * (int64_t)M;
        const float saved = chunked_tree_sum(T, lane, [&](int t) { return pen[clamp_node(act[t], M)]; });
        const float all = chunked_tree_sum(M - 1, lane, [&](int n) { return pen[1 + n]; });
        if (lane == 0) reward[r] = saved - (total + all);
        return;
    }
    if (lane == 0) reward[r] = -total;
}

// 64 rows per 256-thread block; tiles of 64 steps are staged through LDS so that the global reads are
// row-contiguous while thread r still adds row r strictly in step order.
__global__ __launch_bounds__(256) void k_sum_logp(const float* logp, int64_t ld, float* out, int64_t R, int T)
{
    __shared__ float tile[64][65];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    float s = 0.0f;
    for (int t0 = 0; t0 < T; t0 += 64) {
        for (int i = tid; i < 64 * 64; i += 256) {
            const int rr = i >> 6, tt = i & 63;
            const int64_t r = r0 + rr;
            tile[rr][tt] = (r < R && t0 + tt < T) ? logp[r * ld + t0 + tt] : 0.0f;
        }
        __syncthreads();
        if (tid < 64) {
            const int tn = min(64, T - t0);
            for (int t = 0; t < tn; ++t) s = s + tile[tid][t];
        }
        __syncthreads();
    }
    if (tid < 64 && r0 + tid < R) out[r0 + tid] = s;
}

// BeamSearch._make_beam_step (rl4co/utils/decoding.py:573-608): per instance, the beam_width best of the
// beam_width * M candidates  logprobs[w*B + b][n] + parent[w*B + b]  (rows in "(w b)" order), descending; ties go to
// the lower flat index w*M + n.  One workgroup per instance: candidates in LDS, beam_width rounds of a block argmax.
// Output row k*B + b: node, parent beam, cumulative log-prob and the step log-prob of the chosen (beam, node).
__global__ __launch_bounds__(256) void k_beam_topk(const float* logprobs, const float* parent, int64_t B, int BW, int M,
                                                   int64_t* node, int32_t* beam, float* cum, float* step_lp)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* val = reinterpret_cast<float*>(smem);                 // [BW * M]
    float* redv = val + BW * M;                                   // [4]
    int* redi = reinterpret_cast<int*>(redv + 4);                 // [4]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t b = blockIdx.x;
    const int C = BW * M;
    for (int c = tid; c < C; c += 256) {
        const int w = c / M, n = c - w * M;
        const int64_t r = (int64_t)w * B + b;
        val[c] = logprobs[r * M + n] + parent[r];
    }
    __syncthreads();
    for (int k = 0; k < BW; ++k) {
        float best = -INFINITY;
        int besti = 0x7fffffff;
        for (int c = tid; c < C; c += 256) {                      // ascending c per thread: the first maximum is kept
            const float v = val[c];
            if (v == v && (besti == 0x7fffffff || v > best)) { best = v; besti = c; }      // NaN marks "taken"
        }
        wave_argmax(best, besti);
        if (lane == 0) { redv[wv] = best; redi[wv] = besti; }
        __syncthreads();
        if (tid == 0) {
            float bv = redv[0];
            int bi = redi[0];
            for (int i = 1; i < 4; ++i)
                if (redi[i] != 0x7fffffff && (bi == 0x7fffffff || redv[i] > bv || (redv[i] == bv && redi[i] < bi))) { bv = redv[i]; bi = redi[i]; }
            if (bi == 0x7fffffff) bi = 0;                          // unreachable for BW <= BW * M
            const int w = bi / M, n = bi - w * M;
            const int64_t r = (int64_t)k * B + b;
            node[r] = n;
            beam[r] = w;
            cum[r] = bv;
            step_lp[r] = logprobs[((int64_t)w * B + b) * M + n];
            val[bi] = __builtin_nanf("");                          // taken
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The env state BEFORE every decode step of given action rows, in one launch (depot envs; TSP is closed-form in the
// actions: k_tsp_mask_bits): a wavefront keeps its row's state in LDS and alternates "record" (mask as a 128-bit set,
// current node, state scalars) and the env's own transition -- the very row functions of the step kernels above.
// Replaces T x (pack bits, copy current node, state scalar, step) launches of the re-evaluation's set-up.
// ---------------------------------------------------------------------------------------------------------------------
struct ReplayArgs {
    const uint8_t* mask; const uint8_t* visited; const float* used; const float* vcap; const int64_t* cur; const int64_t* istep;
    const float* time; const float* demand; const float* locs; const float* tw; const float* dur;
    const int64_t* actions; uint32_t* bits; int32_t* idxA; float* sc;
    int64_t R, B; int M, T;
};

// SLOTS = 128: graphs up to 112 nodes, masks as one 128-bit word per (row, step).  SLOTS = 1024: larger graphs, masks in the layout
// of the key-chunked re-evaluation kernels -- bits [R][T][nkc][4], nkc = ceil(M / 112), bit i of chunk c = node 112 c + i.
template <int ENV, int SLOTS = 128>
__global__ __launch_bounds__(EB) void k_replay_states(ReplayArgs a)
{
    __shared__ uint8_t s_mask[ROWS_PER_BLOCK][SLOTS], s_vis[ROWS_PER_BLOCK][SLOTS], s_done[ROWS_PER_BLOCK][8];
    __shared__ float s_used[ROWS_PER_BLOCK], s_time[ROWS_PER_BLOCK];
    __shared__ int64_t s_cur[ROWS_PER_BLOCK], s_istep[ROWS_PER_BLOCK];
    const auto [lane, wv, r, live] = wave_row(a.R);
    if (!live) return;
    const int M = a.M, T = a.T;
    const int64_t bi = r % a.B;
    for (int n = lane; n < SLOTS; n += 64) {
        s_mask[wv][n] = n < M ? a.mask[r * M + n] : 0;
        s_vis[wv][n] = n < M ? a.visited[r * M + n] : 0;
    }
    const int nkc = (M + 111) / 112;
    if (lane == 0) {
        s_used[wv] = a.used[r];
        s_time[wv] = a.time ? a.time[r] : 0.0f;
        s_cur[wv] = a.cur[r];
        s_istep[wv] = a.istep ? a.istep[r] : 0;
        s_done[wv][0] = 0;
    }
    __builtin_amdgcn_wave_barrier();
    const float vc = a.vcap[r];
    for (int t = 0; t < T; ++t) {
        // ---- record ------------------------------------------------------------------------------------------------------
        const unsigned long long b0 = __ballot(s_mask[wv][lane] != 0), b1 = __ballot(s_mask[wv][64 + lane] != 0);
        if (SLOTS > 128) {          // one 32-bit word of one chunk per lane
            for (int wi = lane; wi < 4 * nkc; wi += 64) {
                const int c = wi >> 2, w = wi & 3;
                uint32_t v = 0;
                for (int i = 0; i < 32; ++i) {
                    const int li = 32 * w + i, n = 112 * c + li;
                    if (li < 112 && n < M && s_mask[wv][n]) v |= 1u << i;
                }
                a.bits[((r * T + t) * nkc + c) * 4 + w] = v;
            }
        }
        if (lane == 0) {
            const int64_t q = r * T + t;
            if (SLOTS == 128)
                *reinterpret_cast<uint4*>(a.bits + q * 4) =
                    make_uint4((uint32_t)b0, (uint32_t)(b0 >> 32), (uint32_t)b1, (uint32_t)(b1 >> 32));
            a.idxA[q] = (int32_t)s_cur[wv];
            float free_ = vc - s_used[wv];            // free capacity / prize still to collect / length still allowed
            if (ENV == EAMRL_ENV_PCTSP) free_ = free_ < 0.0f ? 0.0f : free_;
            a.sc[q] = free_;
            if (ENV == EAMRL_ENV_CVRPTW) a.sc[a.R * (int64_t)T + q] = s_time[wv];
        }
        __builtin_amdgcn_wave_barrier();
        // ---- the env transition (+ next mask) ---------------------------------------------------------------------------
        const int64_t act = a.actions[r * T + t];
        if (ENV == EAMRL_ENV_CVRP)
            cvrp_step_mask_row<1>(s_vis[wv], &s_used[wv], &vc, a.demand, &s_cur[wv], s_mask[wv], s_done[wv], M - 1, 0, bi, lane, act);
        else if (ENV == EAMRL_ENV_CVRPTW)
            cvrptw_step_mask_row<1>(s_vis[wv], &s_used[wv], &vc, a.demand, &s_cur[wv], &s_time[wv], a.locs, a.tw, a.dur, s_mask[wv],
                                    s_done[wv], M - 1, 0, bi, lane, act);
        else if (ENV == EAMRL_ENV_PCTSP)
            pctsp_step_mask_row<1>(s_vis[wv], &s_used[wv], nullptr, a.demand, nullptr, &s_cur[wv], &s_istep[wv], s_mask[wv], s_done[wv],
                                   M, 0, bi, lane, act);
        else
            op_step_mask_row<1>(s_vis[wv], &s_used[wv], nullptr, nullptr, a.locs, a.demand, &s_cur[wv], &s_istep[wv], s_mask[wv],
                                s_done[wv], M, 0, bi, lane, act);
        __builtin_amdgcn_wave_barrier();
    }
}

// SDVRP: the same recording for SDVRPEnv (sdvrp/env.py:58-92,137-146) -- the state is the remaining-demand row itself, kept in
// registers (nodes lane and lane + 64); additionally every step's row goes to rem_out [R][T][128] (zero padded), which is what the
// re-evaluation's dynamic embedding multiplies.  Arithmetic of k_sdvrp_step_mask.
__global__ __launch_bounds__(EB) void k_replay_sdvrp(const float* __restrict__ rem, const float* __restrict__ used,
                                                     const float* __restrict__ vcap, const int64_t* __restrict__ cur,
                                                     const int64_t* __restrict__ actions, uint32_t* __restrict__ bits,
                                                     int32_t* __restrict__ idxA, float* __restrict__ sc, float* __restrict__ rem_out,
                                                     int64_t R, int M, int T)
{
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    const int n0 = lane, n1 = lane + 64;
    float r0 = n0 < M ? rem[r * M + n0] : 0.0f, r1 = n1 < M ? rem[r * M + n1] : 0.0f;
    float u = used[r];
    const float cap = vcap[r];
    int c = (int)cur[r];
    for (int t = 0; t < T; ++t) {
        // ---- record: mask (get_action_mask), current node, free capacity, the remaining demands -------------------------------
        const bool full = rule::sdvrp_full(u, cap);
        const bool ok0 = n0 >= 1 && n0 < M && !rule::sdvrp_blocked(r0, full), ok1 = n1 < M && !rule::sdvrp_blocked(r1, full);
        unsigned long long b0 = __ballot(ok0), b1 = __ballot(ok1);
        const bool any_free = (b0 | b1) != 0ull;
        if (rule::depot_open(c == 0, any_free)) b0 |= 1ull;                        // the depot
        const int64_t q = r * T + t;
        if (lane == 0) {
            *reinterpret_cast<uint4*>(bits + q * 4) = make_uint4((uint32_t)b0, (uint32_t)(b0 >> 32), (uint32_t)b1, (uint32_t)(b1 >> 32));
            idxA[q] = c;
            sc[q] = cap - u;
        }
        rem_out[q * 128 + n0] = r0;
        rem_out[q * 128 + n1] = r1;
        // ---- SDVRPEnv._step: deliver min(remaining demand, free capacity) ---------------------------------------------------------
        int a = __builtin_amdgcn_readfirstlane((int)actions[q]);
        a = a < 0 ? 0 : (a > M - 1 ? M - 1 : a);
        const float sel = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a < 64 ? r0 : r1), a & 63));
        float left;
        rule::sdvrp_deliver(sel, u, cap, a == 0, u, left);
        if (n0 == a) r0 = left;
        if (n1 == a) r1 = left;
        c = a;
    }
}

// Graphs above 112 nodes (M <= 1024): the row in 16 registers per lane (node lane + 64 k), masks and remaining demands in the
// chunked layout of the key-chunked re-evaluation -- bits [R][T][nkc][4], rem_out [R][T][nkc][128] (ZERO-FILLED by the caller:
// only existing nodes are written), nkc = ceil(M / 112), node n at chunk n / 112, slot n % 112.
__global__ __launch_bounds__(EB) void k_replay_sdvrp_big(const float* __restrict__ rem, const float* __restrict__ used,
                                                         const float* __restrict__ vcap, const int64_t* __restrict__ cur,
                                                         const int64_t* __restrict__ actions, uint32_t* __restrict__ bits,
                                                         int32_t* __restrict__ idxA, float* __restrict__ sc, float* __restrict__ rem_out,
                                                         int64_t R, int M, int T)
{
    __shared__ uint8_t s_ok[ROWS_PER_BLOCK][1024];
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    const int nkc = (M + 111) / 112;
    float rr[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) rr[k] = (lane + 64 * k) < M ? rem[r * M + lane + 64 * k] : 0.0f;
    float u = used[r];
    const float cap = vcap[r];
    int c = (int)cur[r];
    for (int t = 0; t < T; ++t) {
        const int64_t q = r * T + t;
        const bool full = rule::sdvrp_full(u, cap);
        bool any_free = false;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int n = lane + 64 * k;
            const bool ok = n >= 1 && n < M && !rule::sdvrp_blocked(rr[k], full);
            s_ok[wv][n] = ok;
            any_free |= __ballot(ok) != 0ull;
            if (n < M) rem_out[(q * nkc + n / 112) * 128 + n % 112] = rr[k];
        }
        if (lane == 0) {
            s_ok[wv][0] = rule::depot_open(c == 0, any_free);                        // the depot
            idxA[q] = c;
            sc[q] = cap - u;
        }
        __builtin_amdgcn_wave_barrier();
        for (int wi = lane; wi < 4 * nkc; wi += 64) {                      // one 32-bit word of one chunk per lane
            const int ch = wi >> 2, w = wi & 3;
            uint32_t v = 0;
            for (int i = 0; i < 32; ++i) {
                const int li = 32 * w + i, n = 112 * ch + li;
                if (li < 112 && n < M && s_ok[wv][n]) v |= 1u << i;
            }
            bits[(q * nkc + ch) * 4 + w] = v;
        }
        __builtin_amdgcn_wave_barrier();
        // ---- SDVRPEnv._step ------------------------------------------------------------------------------------------------------
        int a = __builtin_amdgcn_readfirstlane((int)actions[q]);
        a = a < 0 ? 0 : (a > M - 1 ? M - 1 : a);
        float selv = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if ((a >> 6) == k) selv = rr[k];
        const float sel = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, selv), a & 63));
        float left;
        rule::sdvrp_deliver(sel, u, cap, a == 0, u, left);
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (lane + 64 * k == a) rr[k] = left;
        c = a;
    }
}

int launch_replay_sdvrp(const float* rem, const float* used, const float* vcap, const int64_t* cur, const int64_t* actions,
                        uint32_t* bits, int32_t* idxA, float* sc, float* rem_out, int64_t R, int M, int T, hipStream_t st)
{
    return launch_rows(M > 112 ? k_replay_sdvrp_big : k_replay_sdvrp, R, st, rem, used, vcap, cur, actions, bits, idxA, sc, rem_out,
                       R, M, T);
}

// TSPEnv / CVRPEnv.check_solution_validity of a row (M <= 4096 nodes): every node (CVRP: every customer; the depot may repeat)
// exactly once, then the CVRP load.  bad[0] += rows that fail the first, bad[1] += valid rows whose load exceeds the capacity.
__device__ __forceinline__ void check_tsp_cvrp_row(SeenBits seen, const int64_t* act, int T, int M, bool with_depot,
                                                   const float* dem, const float* cap_r, int32_t* bad, int lane)
{
    seen.clear(128, lane);
    int bad_lane = 0;
    for (int t = lane; t < T; t += 64) {
        const int64_t a = act[t];
        if (a < 0 || a >= M) { bad_lane = 1; continue; }
        if (with_depot && a == 0) continue;
        if (seen.mark(a)) bad_lane = 1;
    }
    bad_lane |= seen.misses(with_depot ? 1 : 0, M - 1, lane);
    if (__ballot(bad_lane != 0) != 0ull) {
        if (lane == 0) atomicAdd(&bad[0], 1);
        return;
    }
    if (with_depot) {
        const float cap = *cap_r;
        if (cvrp_overloaded(act, dem, cap, cap + 1e-5f, T, lane) && lane == 0) atomicAdd(&bad[1], 1);
    }
}

__global__ __launch_bounds__(EB) void k_check_solution(int env, const int64_t* actions, const float* demand,
                                                       const float* vcap, int64_t R, int64_t B, int N, int T,
                                                       int32_t* bad)
{
    __shared__ uint32_t seen_all[ROWS_PER_BLOCK][128];
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    const bool with_depot = env != EAMRL_ENV_TSP;
    check_tsp_cvrp_row(SeenBits{seen_all[wv]}, actions + r * T, T, with_depot ? N + 1 : N, with_depot,
                       with_depot ? demand + (r % B) * N : nullptr, vcap + r, bad, lane);
}

// ---------------------------------------------------------------------------------------------------------------------
// Rollout epilogue in one launch (TSP / CVRP): the reward, the log-likelihood (in the order of k_sum_logp) and the validity
// (the row function of k_check_solution) of a row by one wavefront; each output is optional.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EB) void k_rollout_finish(int env, const float* locs, const int64_t* actions, const float* logp,
                                                       int64_t ld, const float* demand, const float* vcap, float* reward,
                                                       float* ll, int32_t* bad, int64_t R, int64_t B, int M, int T)
{
    __shared__ uint32_t seen_all[ROWS_PER_BLOCK][128];
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    const bool with_depot = env != EAMRL_ENV_TSP;
    const int64_t* act = actions + r * T;
    const int64_t bi = r % B;
    if (reward) {
        const float length = closed_tour_length(locs + bi * (int64_t)M * 2, act, T, M, with_depot, lane);
        if (lane == 0) reward[r] = -length;
    }
    if (ll) {
        const float s = sum_in_order(logp + r * ld, T, lane);
        if (lane == 0) ll[r] = s;
    }
    if (bad) check_tsp_cvrp_row(SeenBits{seen_all[wv]}, act, T, M, with_depot, demand + bi * (M - 1), vcap + r, bad, lane);
}

// ---------------------------------------------------------------------------------------------------------------------
// Several small device copies / zero fills in one launch (state clones and output buffers of a rollout, the input
// refresh of a replayed graph): blockIdx.y = segment, 16-byte vectors where both ends are aligned.
// ---------------------------------------------------------------------------------------------------------------------
struct MultiCopyArgs { const char* src[EAMRL_MULTI_COPY_MAX]; char* dst[EAMRL_MULTI_COPY_MAX]; int64_t bytes[EAMRL_MULTI_COPY_MAX]; };

__global__ __launch_bounds__(256) void k_multi_copy(MultiCopyArgs a)
{
    const int seg = blockIdx.y;
    const char* src = a.src[seg];
    char* dst = a.dst[seg];
    const int64_t n = a.bytes[seg];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool vec = (((uintptr_t)dst | (uintptr_t)src) & 15) == 0;
    const int64_t nv = vec ? n >> 4 : 0;
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (int64_t i = i0; i < nv; i += stride)
        reinterpret_cast<uint4*>(dst)[i] = src ? reinterpret_cast<const uint4*>(src)[i] : z;
    for (int64_t i = (nv << 4) + i0; i < n; i += stride) dst[i] = src ? src[i] : (char)0;
}

// The step launchers pick STEP once: 1 (transition, then mask) with an action, 0 (mask only) without.
int launch_tsp_step(uint8_t* mask, int64_t* first, int64_t* cur, int64_t* istep, const int64_t* action,
                    uint8_t* done, int64_t R, int N, hipStream_t st)
{
    return launch_rows(k_tsp_step, R, st, mask, first, cur, istep, action, done, R, N);
}

int launch_cvrp(int step, uint8_t* visited, float* used, const float* vcap, const float* demand, int64_t* cur,
                const int64_t* action, uint8_t* mask, uint8_t* done, int64_t R, int64_t B, int N, hipStream_t st)
{
    return launch_rows(step ? k_cvrp_step_mask<1> : k_cvrp_step_mask<0>, R, st, visited, used, vcap, demand, cur, action, mask,
                       done, R, B, N);
}

int launch_sdvrp(float* rem, float* used, const float* vcap, int64_t* cur, const int64_t* action, uint8_t* mask,
                 uint8_t* done, int64_t R, int M, hipStream_t st)
{
    return launch_rows(action ? k_sdvrp_step_mask<1> : k_sdvrp_step_mask<0>, R, st, rem, used, vcap, cur, action, mask, done, R, M);
}

int launch_cvrptw(uint8_t* visited, float* used, const float* vcap, const float* demand, int64_t* cur, float* time,
                  const float* locs, const float* tw, const float* dur, const int64_t* action, uint8_t* mask, uint8_t* done,
                  int64_t R, int64_t B, int N, hipStream_t st)
{
    return launch_rows(action ? k_cvrptw_step_mask<1> : k_cvrptw_step_mask<0>, R, st, visited, used, vcap, demand, cur, time, locs,
                       tw, dur, action, mask, done, R, B, N);
}

int launch_cvrptw_check(const int64_t* actions, const float* locs, const float* tw, const float* dur, int64_t R, int64_t B,
                        int M, int T, int32_t* bad, hipStream_t st)
{
    hipLaunchKernelGGL(k_check_cvrptw_time, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, actions, locs, tw, dur, R, B,
                       M, T, bad);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

int launch_op(uint8_t* visited, float* tour_len, float* prize_tot, const float* prize, const float* locs, const float* maxlen,
              int64_t* cur, int64_t* istep, const int64_t* action, uint8_t* mask, uint8_t* done, int64_t R, int64_t B, int M,
              hipStream_t st)
{
    return launch_rows(action ? k_op_step_mask<1> : k_op_step_mask<0>, R, st, visited, tour_len, prize_tot, prize, locs, maxlen,
                       cur, istep, action, mask, done, R, B, M);
}

int launch_op_reward(const float* prize, const int64_t* actions, float* reward, int64_t R, int64_t B, int M, int T,
                     hipStream_t st)
{
    return launch_rows(k_op_reward, R, st, prize, actions, reward, R, B, M, T);
}

int launch_op_check(const int64_t* actions, const float* locs, const float* maxlen, int64_t R, int64_t B, int M, int T,
                    int32_t* bad, hipStream_t st)
{
    return launch_rows(k_check_op, R, st, actions, locs, maxlen, R, B, M, T, bad);
}

int launch_pctsp(uint8_t* visited, float* prize_tot, float* pen_tot, const float* prize, const float* penalty, int64_t* cur,
                 int64_t* istep, const int64_t* action, uint8_t* mask, uint8_t* done, int64_t R, int64_t B, int M,
                 hipStream_t st)
{
    return launch_rows(action ? k_pctsp_step_mask<1> : k_pctsp_step_mask<0>, R, st, visited, prize_tot, pen_tot, prize, penalty,
                       cur, istep, action, mask, done, R, B, M);
}

int launch_tour_length(const float* locs, const int64_t* actions, float* reward, int64_t R, int64_t B, int M, int T,
                       int with_depot, hipStream_t st, const float* penalty)
{
    return launch_rows(k_tour_length, R, st, locs, actions, reward, R, B, M, T, with_depot, penalty);
}

int launch_sum_logp(const float* logp, int64_t ld, float* out, int64_t R, int T, hipStream_t st)
{
    hipLaunchKernelGGL(k_sum_logp, dim3((unsigned)((R + 63) / 64)), dim3(256), 0, st, logp, ld, out, R, T);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

int launch_replay_states(int env, const uint8_t* mask, const uint8_t* visited, const float* used, const float* vcap,
                         const int64_t* cur, const int64_t* istep, const float* time, const float* demand, const float* locs,
                         const float* tw, const float* dur, const int64_t* actions, uint32_t* bits, int32_t* idxA, float* sc,
                         int64_t R, int64_t B, int M, int T, hipStream_t st)
{
    ReplayArgs a{mask, visited, used, vcap, cur, istep, time, demand, locs, tw, dur, actions, bits, idxA, sc, R, B, M, T};
    const bool big = M > 112;   // the chunked mask layout (graphs above 112 nodes)
    void (*k)(ReplayArgs);
    if (env == EAMRL_ENV_CVRP) k = big ? k_replay_states<EAMRL_ENV_CVRP, 1024> : k_replay_states<EAMRL_ENV_CVRP>;
    else if (env == EAMRL_ENV_CVRPTW) k = big ? k_replay_states<EAMRL_ENV_CVRPTW, 1024> : k_replay_states<EAMRL_ENV_CVRPTW>;
    else if (env == EAMRL_ENV_PCTSP) k = big ? k_replay_states<EAMRL_ENV_PCTSP, 1024> : k_replay_states<EAMRL_ENV_PCTSP>;
    else if (env == EAMRL_ENV_OP) k = big ? k_replay_states<EAMRL_ENV_OP, 1024> : k_replay_states<EAMRL_ENV_OP>;
    else return EAMRL_E_ARG;
    return launch_rows(k, R, st, a);
}

int launch_rollout_finish(int env, const float* locs, const int64_t* actions, const float* logp, int64_t ld, const float* demand,
                          const float* vcap, float* reward, float* ll, int32_t* bad, int64_t R, int64_t B, int M, int T,
                          hipStream_t st)
{
    return launch_rows(k_rollout_finish, R, st, env, locs, actions, logp, ld, demand, vcap, reward, ll, bad, R, B, M, T);
}

int launch_multi_copy(int n, const void* const* src, void* const* dst, const int64_t* bytes, hipStream_t st)
{
    MultiCopyArgs a;
    int64_t mx = 0;
    int m = 0;
    for (int i = 0; i < n; ++i) {
        if (bytes[i] <= 0) continue;
        a.src[m] = (const char*)src[i]; a.dst[m] = (char*)dst[i]; a.bytes[m] = bytes[i];
        mx = bytes[i] > mx ? bytes[i] : mx;
        ++m;
    }
    if (m == 0) return 0;
    int64_t bx = (mx / 16 + 255) / 256;
    bx = bx < 1 ? 1 : (bx > 2048 ? 2048 : bx);
    hipLaunchKernelGGL(k_multi_copy, dim3((unsigned)bx, (unsigned)m), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

int launch_beam_topk(const float* logprobs, const float* parent, int64_t B, int BW, int M, int64_t* node, int32_t* beam,
                     float* cum, float* step_lp, hipStream_t st)
{
    const size_t lds = ((size_t)BW * M + 8) * sizeof(float);
    if (lds > 150 * 1024) return EAMRL_E_ARG;
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(k_beam_topk),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return EAMRL_E_LAUNCH;
    hipLaunchKernelGGL(k_beam_topk, dim3((unsigned)B), dim3(256), lds, st, logprobs, parent, B, BW, M, node, beam, cum, step_lp);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

int launch_check_solution(int env, const int64_t* actions, const float* demand, const float* vcap, int64_t R, int64_t B,
                          int N, int T, int32_t* bad, hipStream_t st)
{
    if (N + 1 > 4096) return EAMRL_E_ARG;
    if (env == EAMRL_ENV_PCTSP) return launch_rows(k_check_pctsp, R, st, actions, demand, R, B, N + 1, T, bad);      // real_prize [B][N+1]
    if (env == EAMRL_ENV_SDVRP) {
        const size_t lds = (size_t)ROWS_PER_BLOCK * (N + 1) * sizeof(float);
        if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(k_check_sdvrp),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return EAMRL_E_LAUNCH;
        hipLaunchKernelGGL(k_check_sdvrp, dim3(row_blocks(R)), dim3(EB), lds, st, actions, demand, vcap, R, B, N, T, bad);
        return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
    }
    return launch_rows(k_check_solution, R, st, env, actions, demand, vcap, R, B, N, T, bad);
}

}  // namespace eamrl
