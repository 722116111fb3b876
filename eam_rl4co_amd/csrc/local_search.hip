// TSP local search: best-improvement 2-opt, the whole sweep loop of a tour in one launch.
//
//   k_two_opt   TSPEnv.local_search -> two_opt_once / _two_opt_python   rl4co/envs/routing/tsp/local_search.py:17-79
//
// One workgroup per tour.  A sweep scans every pair 1 <= i < j <= n-1 of tour positions for
//     change = ((d[t[i-1]][t[j]] + d[t[i]][t[j+1]]) - d[t[i-1]][t[i]]) - d[t[j]][t[j+1]]        (float32, this order; t[n] = t[0])
// takes the first minimum in (i, j) scan order among the negative ones and, if it is below -1e-6, reverses positions i..j;
// the loop ends after the first sweep that reverses nothing, or at max_iterations.
//
// LDS keeps the tour, the current edge lengths e[k] = d[t[k-1]][t[k]] (k = 1..n; slot n closes the tour: position 0 never
// moves, so t[n] = t[0] is a fixed sentinel) and
//   COORDS:        the coordinates in TOUR ORDER, so a candidate reads positions i-1, i, j, j+1 (lane-consecutive j: conflict-free)
//                  and costs two square roots; d is the project's canonical leg sqrtf(fmaf(dy, dy, dx * dx)) (OP),
//                  bit for bit torch's norm(p=2, dim=-1) behind the reference's get_distance_matrix -- no N x N matrix exists;
//   MATRIX_LDS:    the caller's distance matrix, staged once (4 n^2 bytes, n <= EAMRL_TWO_OPT_LDS_MATRIX_MAX);
//   MATRIX_GLOBAL: the caller's matrix read from global memory (cache-resident: 4 MB per tour at n = 1024).
// The triangle of pairs is folded into a rectangle (row i next to row n-1-i: n-1 candidates together) and dealt to the threads
// linearly, so every lane has work whatever n is.  The arg-min is a 64-bit max of (bits(change) << 32 | ~(i n + j)): among negative
// floats a larger bit pattern is a smaller value, and the inverted pair index sends ties to the first pair in scan order.
#include "kernels.hpp"

namespace eamrl {

enum { TWO_OPT_COORDS = 0, TWO_OPT_MATRIX_LDS = 1, TWO_OPT_MATRIX_GLOBAL = 2 };

// the canonical leg (env_rule.hpp rule::leg)
__device__ __forceinline__ float leg2(float2 a, float2 b)
{
    const float dx = a.x - b.x, dy = a.y - b.y;
    return __builtin_sqrtf(fma_(dy, dy, dx * dx));
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

// dynamic LDS: red [16] u64 | e [n+1] f32 | t [n+1] i32 | seen [32] u32 | COORDS: P [n+1] float2, MATRIX_LDS: D [n*n] f32
// (the tail starts at 256 + 8 (n+1) bytes: 8-byte aligned)
static size_t two_opt_lds_bytes(int n, int mode)
{
    return 16 * 8 + (size_t)(n + 1) * 4 + (size_t)(n + 1) * 4 + 32 * 4 +
           (mode == TWO_OPT_COORDS ? (size_t)(n + 1) * 8 : mode == TWO_OPT_MATRIX_LDS ? (size_t)n * n * 4 : 0);
}

template <int NT, int MODE>
__global__ __launch_bounds__(NT) void k_two_opt(const float* __restrict__ locs, const float* __restrict__ distances,
                                                const int64_t* __restrict__ actions_in, int64_t* __restrict__ actions_out,
                                                int32_t* __restrict__ iters, int32_t* __restrict__ status, int n,
                                                int max_iterations)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long* red = reinterpret_cast<unsigned long long*>(smem);
    float* e = reinterpret_cast<float*>(red + 16);
    int* t = reinterpret_cast<int*>(e + (n + 1));
    uint32_t* seen = reinterpret_cast<uint32_t*>(t + (n + 1));
    float2* P = reinterpret_cast<float2*>(seen + 32);       // COORDS only
    float* Dl = reinterpret_cast<float*>(seen + 32);        // MATRIX_LDS only

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int NW = NT / 64;
    const int64_t b = blockIdx.x;
    const int64_t* ain = actions_in + b * n;
    int64_t* aout = actions_out + b * n;
    const float* L = MODE == TWO_OPT_COORDS ? locs + b * (int64_t)n * 2 : nullptr;
    const float* Dg = MODE == TWO_OPT_COORDS ? nullptr : distances + b * (int64_t)n * n;

    // ---- the row must be a permutation of 0..n-1: otherwise it is copied through and counted ---------------------------------
    if (tid < 32) seen[tid] = 0;
    __syncthreads();
    int bad = 0;
    for (int k = tid; k < n; k += NT) {
        const int64_t a = ain[k];
        if (a < 0 || a >= n) { bad = 1; continue; }
        const uint32_t bit = 1u << (a & 31);
        if (atomicOr(&seen[a >> 5], bit) & bit) bad = 1;
        t[k] = (int)a;
    }
    if (__syncthreads_or(bad)) {                       // n distinct values inside 0..n-1 are all of them
        for (int k = tid; k < n; k += NT) aout[k] = ain[k];
        if (tid == 0) { iters[b] = 0; atomicAdd(status, 1); }
        return;
    }
    if (tid == 0) t[n] = t[0];
    if (MODE == TWO_OPT_MATRIX_LDS)
        for (int k = tid; k < n * n; k += NT) Dl[k] = Dg[k];
    if (MODE == TWO_OPT_COORDS)
        for (int k = tid; k <= n; k += NT) {
            const int a = t[k == n ? 0 : k];
            P[k] = make_float2(L[2 * a], L[2 * a + 1]);
        }
    __syncthreads();
    auto dm = [&](int a, int c) -> float { return MODE == TWO_OPT_MATRIX_LDS ? Dl[a * n + c] : Dg[(int64_t)a * n + c]; };
    auto edge = [&](int k) -> float { return MODE == TWO_OPT_COORDS ? leg2(P[k - 1], P[k]) : dm(t[k - 1], t[k]); };
    for (int k = 1 + tid; k <= n; k += NT) e[k] = edge(k);
    __syncthreads();

    // folded pair rectangle: F rows of W candidates; row f = the pairs of i = 1 + f (its first n-2-f columns) and of i = n-2-f
    const int W = n - 1, F = (n - 1) / 2, total = F * W;
    const int qs = NT / W, rs = NT - qs * W;           // W >= 1 (n >= 2)
    const int f0 = tid / W, c0 = tid - f0 * W;

    int sweeps = 0;
    while (sweeps < max_iterations) {
        unsigned long long best = 0ull;
        int f = f0, c = c0;
        for (int idx = tid; idx < total; idx += NT) {
            const int iA = 1 + f, iB = n - 2 - f, lenA = n - 2 - f;
            const bool inA = c < lenA;
            const int i = inA ? iA : iB;
            const int j = inA ? iA + 1 + c : iB + 1 + (c - lenA);
            if (inA || iA != iB) {                     // the middle row of an odd triangle has no partner
                float first, second;
                if (MODE == TWO_OPT_COORDS) {
                    first = leg2(P[i - 1], P[j]);
                    second = leg2(P[i], P[j + 1]);
                } else {
                    first = dm(t[i - 1], t[j]);
                    second = dm(t[i], t[j + 1]);
                }
                const float change = ((first + second) - e[i]) - e[j + 1];
                if (change < 0.0f) {
                    const unsigned long long key =
                        ((unsigned long long)__float_as_uint(change) << 32) | (0xffffffffu - (unsigned)(i * n + j));
                    best = key > best ? key : best;
                }
            }
            f += qs;
            c += rs;
            if (c >= W) { c -= W; ++f; }
        }
        best = wave_max_u64(best);
        if (NW > 1) {
            if (lane == 0) red[wv] = best;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const unsigned long long o = red[w];
                best = o > best ? o : best;
            }
        }
        ++sweeps;
        const float delta = best ? __uint_as_float((unsigned)(best >> 32)) : 0.0f;
        if (!(delta < -1e-6f)) break;
        const int pair = (int)(0xffffffffu - (unsigned)best);
        const int p = pair / n, q = pair - p * n;
        // ---- reverse positions p..q (disjoint swaps), then refresh the edges that end in p..q+1 -----------------------------
        const int half = (q - p + 1) >> 1;
        for (int k = tid; k < half; k += NT) {
            const int x = p + k, y = q - k;
            const int tx = t[x];
            t[x] = t[y];
            t[y] = tx;
            if (MODE == TWO_OPT_COORDS) {
                const float2 px = P[x];
                P[x] = P[y];
                P[y] = px;
            }
        }
        __syncthreads();
        for (int k = p + tid; k <= q + 1; k += NT) e[k] = edge(k);
        __syncthreads();
    }
    for (int k = tid; k < n; k += NT) aout[k] = t[k];
    if (tid == 0) iters[b] = sweeps;
}

template <int NT, int MODE>
static int launch_two_opt_as(const float* locs, const float* distances, const int64_t* actions_in, int64_t* actions_out,
                             int32_t* iters, int32_t* status, int64_t B, int N, int max_iterations, hipStream_t st)
{
    hipLaunchKernelGGL((k_two_opt<NT, MODE>), dim3((unsigned)B), dim3(NT), two_opt_lds_bytes(N, MODE), st, locs, distances,
                       actions_in, actions_out, iters, status, N, max_iterations);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

// one wavefront up to EAMRL_TWO_OPT_WAVE_MAX nodes (no cross-wavefront step), four up to EAMRL_TWO_OPT_BLOCK256_MAX, sixteen above
template <int MODE>
static int launch_two_opt_mode(const float* locs, const float* distances, const int64_t* actions_in, int64_t* actions_out,
                               int32_t* iters, int32_t* status, int64_t B, int N, int max_iterations, hipStream_t st)
{
    if (N <= EAMRL_TWO_OPT_WAVE_MAX)
        return launch_two_opt_as<64, MODE>(locs, distances, actions_in, actions_out, iters, status, B, N, max_iterations, st);
    if (N <= EAMRL_TWO_OPT_BLOCK256_MAX)
        return launch_two_opt_as<256, MODE>(locs, distances, actions_in, actions_out, iters, status, B, N, max_iterations, st);
    return launch_two_opt_as<1024, MODE>(locs, distances, actions_in, actions_out, iters, status, B, N, max_iterations, st);
}

int launch_tsp_two_opt(const float* locs, const float* distances, const int64_t* actions_in, int64_t* actions_out,
                       int32_t* iters, int32_t* status, int64_t B, int N, int max_iterations, hipStream_t st)
{
    if (N < 2 || N > 1024 || B < 1 || B > 0x7fffffff || max_iterations < 0) return EAMRL_E_ARG;
    if (!distances)
        return launch_two_opt_mode<TWO_OPT_COORDS>(locs, distances, actions_in, actions_out, iters, status, B, N, max_iterations, st);
    if (N <= EAMRL_TWO_OPT_LDS_MATRIX_MAX)         // N = 120: 57,600 + 8 * 121 + 256 = 58,824 bytes of the 65,536 (126 would still fit)
        return launch_two_opt_mode<TWO_OPT_MATRIX_LDS>(locs, distances, actions_in, actions_out, iters, status, B, N,
                                                       max_iterations, st);
    return launch_two_opt_mode<TWO_OPT_MATRIX_GLOBAL>(locs, distances, actions_in, actions_out, iters, status, B, N, max_iterations,
                                                      st);
}

}  // namespace eamrl
