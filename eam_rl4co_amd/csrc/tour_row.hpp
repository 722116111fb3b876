// What one 64-lane wavefront computes about one row of a tour, stated once: the row a wavefront owns, the chunked lane-tree
// sum, the closed tour length, the "seen" bitmap of the validity checks, the strictly sequential replays, and the launch of
// such a kernel.  The kernels of env_reward.hip and pdp.hip and the fitness sums of evolution_common.hpp are built on these;
// the env comparisons themselves (and the leg) are env_rule.hpp's.
#pragma once
#include "kernels.hpp"
#include "env_rule.hpp"

namespace eamrl {

constexpr int EB = 256;          // threads per block
constexpr int ROWS_PER_BLOCK = EB / 64;

struct WaveRow { int lane, wv; int64_t r; bool live; };

// the row of this wavefront in a grid of rows_per_block-wavefront blocks; live: the row exists
__device__ __forceinline__ WaveRow wave_row(int64_t R, int rows_per_block = ROWS_PER_BLOCK)
{
    const int wv = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * rows_per_block + wv;
    return {(int)(threadIdx.x & 63), wv, r, r < R};
}

// a caller-supplied node id, kept inside the instance whatever it is
__device__ __forceinline__ int64_t clamp_node(int64_t a, int M) { return a < 0 ? 0 : (a >= M ? M - 1 : a); }

// sum of f(t), t < n, in the canonical order: 64-blocks ascending, the lane tree inside a block, the first block assigned
// (not added to zero).  Every lane gets the result.
template <class F>
__device__ __forceinline__ float chunked_tree_sum(int n, int lane, F f)
{
    float total = 0.0f;
    for (int b0 = 0; b0 < n; b0 += 64) {
        const int t = b0 + lane;
        const float s = wave_tree_sum(t < n ? f(t) : 0.0f);
        total = (b0 == 0) ? s : total + s;
    }
    return total;
}

// closed tour over act[0..T) of the nodes L [M][2]; with_depot: depot -> act -> depot (T + 1 legs), else act[T-1] -> act[0]
// closes it.  leg(a, b) and leg(b, a) are the same bits: the differences are only squared.
__device__ __forceinline__ float closed_tour_length(const float* L, const int64_t* act, int T, int M, bool with_depot, int lane)
{
    const int P = T + (with_depot ? 1 : 0);
    return chunked_tree_sum(P, lane, [&](int t) {
        int64_t a0, a1;
        if (with_depot) {
            a0 = (t == 0) ? 0 : act[t - 1];
            a1 = (t + 1 == P) ? 0 : act[t];
        } else {
            a0 = act[t];
            a1 = act[(t + 1 == P) ? 0 : t + 1];
        }
        const float2 p0 = *reinterpret_cast<const float2*>(L + 2 * clamp_node(a0, M));
        const float2 p1 = *reinterpret_cast<const float2*>(L + 2 * clamp_node(a1, M));
        return rule::leg(p1.x, p1.y, p0.x, p0.y);
    });
}

// "visited exactly once": one bit per node in a wavefront's own LDS words.  What is out of range, which nodes are skipped and
// what else a mark records is the calling kernel's rule.
struct SeenBits {
    uint32_t* w;
    __device__ __forceinline__ void clear(int words, int lane) const
    {
        for (int i = lane; i < words; i += 64) w[i] = 0;
        __builtin_amdgcn_wave_barrier();
    }
    // -> the node was marked already
    __device__ __forceinline__ bool mark(int64_t a) const
    {
        const uint32_t bit = 1u << (a & 31);
        return (atomicOr(&w[a >> 5], bit) & bit) != 0;
    }
    // after all marks -> this lane found a node of lo..top unmarked
    __device__ __forceinline__ int misses(int lo, int top, int lane) const
    {
        __builtin_amdgcn_wave_barrier();
        int miss = 0;
        for (int n = lo + lane; n <= top; n += 64)
            if (!((w[n >> 5] >> (n & 31)) & 1u)) miss = 1;
        return miss;
    }
};

// step(value(t)) for t = 0 .. T-1 strictly in order: the 64 values of a block are fetched by the lanes at once and consumed
// through v_readlane, every lane running the same chain
template <class V, class S>
__device__ __forceinline__ void for_each_step_in_order(int T, int lane, V value, S step)
{
    for (int t0 = 0; t0 < T; t0 += 64) {
        const float v = (t0 + lane < T) ? value(t0 + lane) : 0.0f;
        const int tn = T - t0 < 64 ? T - t0 : 64;
#pragma unroll
        for (int t = 0; t < 64; ++t)
            if (t < tn) step(__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), t)));
    }
}

// get_log_likelihood of a row: ((0 + logp[0]) + logp[1]) + ...
__device__ __forceinline__ float sum_in_order(const float* logp, int T, int lane)
{
    float s = 0.0f;
    for_each_step_in_order(T, lane, [&](int t) { return logp[t]; }, [&](float v) { s = s + v; });
    return s;
}

// the running load of a CVRP tour over valid ids (cvrp/env.py:172-185): the depot takes the capacity off, the load never goes
// below zero -> it exceeded lim (the caller's cap + tolerance) at some step
__device__ __forceinline__ bool cvrp_overloaded(const int64_t* act, const float* dem, float cap, float lim, int T, int lane)
{
    float usedc = 0.0f;
    int over = 0;
    for_each_step_in_order(
        T, lane,
        [&](int t) {
            const int64_t a = act[t];
            return (a == 0) ? -cap : dem[a - 1];
        },
        [&](float delta) {
            usedc = usedc + delta;
            if (usedc < 0.0f) usedc = 0.0f;
            if (usedc > lim) over = 1;
        });
    return over != 0;
}

static inline unsigned row_blocks(int64_t R) { return (unsigned)((R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK); }

// the launch of a one-wavefront-per-row kernel of EB threads over R rows
template <class K, class... A>
int launch_rows(K kernel, int64_t R, hipStream_t st, A... args)
{
    hipLaunchKernelGGL(kernel, dim3(row_blocks(R)), dim3(EB), 0, st, args...);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

}  // namespace eamrl
