// Pickup-and-delivery (PDP) kernels outside the decode loop: env transition + mask, validity, init embedding.
//
//   k_pdp_step_mask        PDPEnv._step (+ the mask it stores)      rl4co/envs/routing/pdp/env.py:66-106
//   k_check_pdp            PDPEnv.check_solution_validity           rl4co/envs/routing/pdp/env.py:206-226
//   k_pdp_init_embedding   PDPInitEmbedding.forward                 rl4co/models/nn/env_embeddings/init.py:347-372
//
// M = N + 1 nodes: depot 0, pickups 1 .. N/2, deliveries N/2 + 1 .. N; pickup i pairs with delivery i + N/2.  The state is
// two byte sets per row, visited (= !available) and to_deliver; a node is feasible iff it is unvisited and to deliver.
// One 64-lane wavefront per row for the integer kernels, as in env_reward.hip, on the row primitives of tour_row.hpp.
#include "tour_row.hpp"

namespace eamrl {

constexpr int PDP_CHECK_MAX_M = 4096;

// STEP = 0: mask only; STEP = 1: visit `action`, open its partner, then the mask.  The partner index keeps the reference's
// modulo: (a + N/2) % (N + 1) is the delivery of a pickup, and for a delivery (or the depot) it is the depot or a pickup,
// whose to_deliver bit is set already -- written all the same, so that the state equals the reference's.
template <int STEP>
__global__ __launch_bounds__(EB) void k_pdp_step_mask(uint8_t* visited, uint8_t* to_deliver, int64_t* cur, const int64_t* action,
                                                      uint8_t* mask, uint8_t* done, int64_t R, int M)
{
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    uint8_t* vis = visited + r * M;
    uint8_t* td = to_deliver + r * M;
    int64_t a = -1, d = -1;
    if (STEP) {
        a = action[r];
        a = a < 0 ? 0 : (a > M - 1 ? M - 1 : a);      // an out-of-range action must not become an out-of-bounds access
        d = rule::pdp_partner(a, M);
    }
    int all_vis = 1;
    for (int n = lane; n < M; n += 64) {
        int v = vis[n] != 0, t = td[n] != 0;
        if (STEP && n == a) { v = 1; vis[n] = 1; }
        if (STEP && n == d) { t = 1; td[n] = 1; }
        mask[r * M + n] = (!v) & t;
        all_vis &= v;
    }
    const bool allc = __ballot(all_vis == 0) == 0ull;
    if (STEP && lane == 0) {
        cur[r] = a;
        done[r] = allc ? 1 : 0;
    }
}

// bad[0] += rows that are not a permutation of 1 .. N (a repeated or missing node, the depot inside, an id out of range),
// bad[1] += permutations that visit a delivery before its pickup.  T == N: the tour as the default env records it (the
// reference prepends the depot).  T == N + 1 (force_start_at_depot): the tour holds the depot itself, which the reference
// accepts on the first or the last position only.  A row is counted once, for the first assertion it fails.
__global__ __launch_bounds__(EB) void k_check_pdp(const int64_t* actions, int64_t R, int M, int T, int32_t* bad)
{
    __shared__ uint32_t seen_all[ROWS_PER_BLOCK][PDP_CHECK_MAX_M / 32];
    __shared__ uint16_t pos_all[ROWS_PER_BLOCK][PDP_CHECK_MAX_M];
    const auto [lane, wv, r, live] = wave_row(R);
    if (!live) return;
    const SeenBits seen{seen_all[wv]};
    uint16_t* pos = pos_all[wv];
    seen.clear((M + 31) / 32, lane);
    const int64_t* act = actions + r * T;
    const int N = M - 1;
    const bool with0 = T == M;
    int bad_lane = (T != N && T != M);
    for (int t = lane; t < T; t += 64) {
        const int64_t a = act[t];
        if (a < 0 || a > N) { bad_lane = 1; continue; }
        if (a == 0 && !(with0 && (t == 0 || t == T - 1))) { bad_lane = 1; continue; }
        if (seen.mark(a)) bad_lane = 1;      // visited twice
        else pos[a] = (uint16_t)t;
    }
    bad_lane |= seen.misses(with0 ? 0 : 1, N, lane);      // never visited
    const bool invalid = __ballot(bad_lane != 0) != 0ull;
    if (invalid) {
        if (lane == 0) atomicAdd(&bad[0], 1);
        return;
    }
    int early = 0;
    for (int i = 1 + lane; i <= N / 2; i += 64) early |= !(pos[i] < pos[i + N / 2]);
    if (__ballot(early != 0) != 0ull && lane == 0) atomicAdd(&bad[1], 1);
}

// h[b][n][e] = bias[e] + chain_k(x[k] * W[e][k]) -- the k-ordered fma chain of eamrl_linear -- with, for node n of instance b,
//   n == 0        x = locs[b][0]                       (Wd [E][2], bd)   init_embed_depot
//   1 <= n <= N/2 x = locs[b][n] | locs[b][n + N/2]    (Wp [E][4], bp)   init_embed_pick: the pickup and its delivery
//   n >  N/2      x = locs[b][n]                       (Wl [E][2], bl)   init_embed_delivery
__global__ __launch_bounds__(EB) void k_pdp_init_embedding(const float* __restrict__ locs, const float* __restrict__ Wd,
                                                           const float* __restrict__ bd, const float* __restrict__ Wp,
                                                           const float* __restrict__ bp, const float* __restrict__ Wl,
                                                           const float* __restrict__ bl, float* __restrict__ h, int64_t B,
                                                           int M, int E)
{
    const int64_t total = B * (int64_t)M * E;
    const int half = (M - 1) / 2;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < total; i += (int64_t)gridDim.x * EB) {
        const int e = (int)(i % E);
        const int64_t bn = i / E;
        const int n = (int)(bn % M);
        const float* x = locs + bn * 2;
        float acc;
        if (n == 0) {
            acc = bd ? bd[e] : 0.0f;
            acc = fma_(x[0], Wd[2 * e], acc);
            acc = fma_(x[1], Wd[2 * e + 1], acc);
        } else if (n <= half) {
            const float* xd = x + 2 * half;
            acc = bp ? bp[e] : 0.0f;
            acc = fma_(x[0], Wp[4 * e], acc);
            acc = fma_(x[1], Wp[4 * e + 1], acc);
            acc = fma_(xd[0], Wp[4 * e + 2], acc);
            acc = fma_(xd[1], Wp[4 * e + 3], acc);
        } else {
            acc = bl ? bl[e] : 0.0f;
            acc = fma_(x[0], Wl[2 * e], acc);
            acc = fma_(x[1], Wl[2 * e + 1], acc);
        }
        h[i] = acc;
    }
}

int launch_pdp(uint8_t* visited, uint8_t* to_deliver, int64_t* cur, const int64_t* action, uint8_t* mask, uint8_t* done, int64_t R,
               int M, hipStream_t st)
{
    return launch_rows(action ? k_pdp_step_mask<1> : k_pdp_step_mask<0>, R, st, visited, to_deliver, cur, action, mask, done, R, M);
}

int launch_pdp_check(const int64_t* actions, int64_t R, int M, int T, int32_t* bad, hipStream_t st)
{
    if (M > PDP_CHECK_MAX_M || T > 0xffff) return EAMRL_E_ARG;
    return launch_rows(k_check_pdp, R, st, actions, R, M, T, bad);
}

int launch_pdp_init_embedding(const float* locs, const float* Wd, const float* bd, const float* Wp, const float* bp,
                              const float* Wl, const float* bl, float* h, int64_t B, int M, int E, hipStream_t st)
{
    const int64_t total = B * (int64_t)M * E;
    int64_t blocks = (total + EB - 1) / EB;
    blocks = blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks);
    hipLaunchKernelGGL(k_pdp_init_embedding, dim3((unsigned)blocks), dim3(EB), 0, st, locs, Wd, bd, Wp, bp, Wl, bl, h, B, M, E);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

}  // namespace eamrl
