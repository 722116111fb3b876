// The fp32 MFMA tile primitives of every kernel file that issues v_mfma_f32_16x16x4_f32: the f32x4 accumulator type and the one
// wrapper of the instruction (mf), the staging of a head's keys and values into MFMA fragment order for the two attention
// forwards (stage_kv_fragments), and what the 16-query-tile kernels (reeval.hip, eas_layer.hip, rollout_multistart.hip, ptrnet.hip,
// moe_ffn.hip) share besides: the A-layout of a staged tile, the query walker and the fragment-order weight stream.
// The cross-lane reductions live in dmath.hpp: lane_groups_sum / lane_groups_max (vmax_raw) over the four lane groups that share
// a query, row_*_dpp over the 16 lanes of a row.  row16_sum below is NOT row_sum_dpp: it goes through __shfl_xor (ds_bpermute),
// other instructions on a hot path, and keeps its own name so that no file can pick the wrong one by include order.
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

// sum over the 16 lanes that share a lane group (the tile's 16 queries), on __shfl_xor (see the header comment)
__device__ __forceinline__ float row16_sum(float v)
{
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    return v;
}

// One head's keys and values in LDS in MFMA fragment order, for the attention forwards that keep the softmax weights in their
// accumulator registers (k_mha_encoder_mfma, k_hetero_mha).  Per 16-key tile kt and lane (j, G) one float4 = the A operand of
// the tile's four k-steps:
//   KF[kt][lane] = { K[16 kt + pi(j)][4 t + G] : t = 0..3 },  pi(j) = 4 (j & 3) + (j >> 2): with the keys of a tile placed on
//                  the MFMA rows in this order the score accumulator register r of lane group G is key 16 kt + 4 r + G, i.e.
//                  the B operand of value k-step r -- the softmax weights never leave their registers;
//   VF[kt][lane] = { V[16 kt + 4 r + G][j] : r = 0..3 }   (V^T: the A operand of the value product, rows = head columns).
// KF, VF: [NT][64][4] floats.  base: the head's first q column of row 0; row n is ld floats on, its 16 key columns at + E, its
// value columns at + 2 E (16-byte aligned).  Thread = key, the whole workgroup; rows n >= N of the NT tiles are zeros.  The
// caller synchronises.
__device__ __forceinline__ void stage_kv_fragments(float* KF, float* VF, const float* base, int64_t ld, int E, int N, int NT)
{
    for (int n = threadIdx.x; n < NT * 16; n += blockDim.x) {
        float kr[16], vr[16];
#pragma unroll
        for (int c = 0; c < 16; c += 4) {
            float4 kk = make_float4(0.f, 0.f, 0.f, 0.f), vv = kk;
            if (n < N) {
                kk = *reinterpret_cast<const float4*>(base + (int64_t)n * ld + E + c);
                vv = *reinterpret_cast<const float4*>(base + (int64_t)n * ld + 2 * E + c);
            }
            kr[c] = kk.x; kr[c + 1] = kk.y; kr[c + 2] = kk.z; kr[c + 3] = kk.w;
            vr[c] = vv.x; vr[c + 1] = vv.y; vr[c + 2] = vv.z; vr[c + 3] = vv.w;
        }
        const int kt = n >> 4, kk = n & 15;
        const int jr = 4 * (kk & 3) + (kk >> 2);        // the MFMA row that carries key kk of its tile (pi is an involution)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(KF + ((size_t)kt * 64 + 16 * g + jr) * 4) = make_float4(kr[g], kr[4 + g], kr[8 + g], kr[12 + g]);
        const int r = kk >> 2, g = kk & 3;              // key 16 kt + 4 r + g: k-step r, lane group g
#pragma unroll
        for (int e = 0; e < 16; ++e) VF[((size_t)kt * 64 + 16 * g + e) * 4 + r] = vr[e];
    }
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
