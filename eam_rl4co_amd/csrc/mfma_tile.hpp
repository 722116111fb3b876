// The fp32 MFMA tile primitives shared by the 16-query-tile kernels (reeval.hip, eas_layer.hip, rollout_multistart.hip): the
// v_mfma_f32_16x16x4_f32 wrapper, the A-layout of a staged tile, the lane-group sums, the query walker and the fragment-order
// weight stream.  Only what those files had token for token in common lives here; group_max does NOT (rollout_multistart.hip is
// bit-exact to the oracle and takes vmax_raw, reeval.hip takes fmaxf): each file keeps its own.
#pragma once
#include "kernels.hpp"

namespace eamrl {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TS = 140, TG = 34;     // A-layout tile buffers [16][TS]: element (j, c) at j * TS + a_off(c)
__device__ __forceinline__ int a_off(int c) { return (c & 3) * TG + (c >> 2); }
constexpr int DS = 17;               // row stride of the du tile ([n][q])
constexpr float LOG2E = 1.44269504088896341f;

__device__ __forceinline__ f32x4 mf(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 z4() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ float fexp(float x) { return __builtin_amdgcn_exp2f(x * LOG2E); }

// sum over the four lane groups (lanes l, l^16, l^32, l^48) that share a query: first the ^16 partner, then the ^32 one
__device__ __forceinline__ float group_sum(float v)
{
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
// sum over the 16 lanes that share a lane group (the tile's 16 queries)
__device__ __forceinline__ float row16_sum(float v)
{
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    return v;
}

struct QWalk {          // query l = first, first + 16, ... of a row chunk as l = sl * T + t
    int sl, t;
    __device__ __forceinline__ void init(int l, int T) { sl = l / T; t = l - sl * T; }
    __device__ __forceinline__ void next(int T)
    {
        t += 16;
        while (t >= T) { t -= T; ++sl; }
    }
};

// fragment-order weight stream (eamrl_polynet, eamrl_eas_layer): a piece = PQ consecutive 16-byte A-fragment loads of one row
// tile = 16 k-steps
constexpr int PQ = 4;
__device__ __forceinline__ void w_load(f32x4 (&dst)[PQ], const float* W, int piece, int lane)
{
    const f32x4* wp = reinterpret_cast<const f32x4*>(W) + piece * (PQ * 64) + lane;
#pragma unroll
    for (int i = 0; i < PQ; ++i) dst[i] = wp[64 * i];
}
// acc0 / acc1 += the piece's A fragments x 16 k-steps of a tile (hp: this lane's row of an A-layout tile, at the piece's first k-step)
__device__ __forceinline__ void w_gemm(const f32x4 (&w)[PQ], const float* hp, f32x4& acc0, f32x4& acc1)
{
#pragma unroll
    for (int i = 0; i < PQ; ++i) {
        const float2 lo = *reinterpret_cast<const float2*>(hp + 4 * i), hi = *reinterpret_cast<const float2*>(hp + 4 * i + 2);
        f32x4& acc = (i & 1) ? acc1 : acc0;
        acc = mf(w[i][0], lo.x, acc); acc = mf(w[i][1], lo.y, acc);
        acc = mf(w[i][2], hi.x, acc); acc = mf(w[i][3], hi.y, acc);
    }
}

}  // namespace eamrl
