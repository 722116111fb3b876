// What the fused encoders k_encoder_fused (encoder_fused.hip, fp32 MFMA) and k_encoder_fused16 (encoder_fused16.hip, 16-bit
// MFMA) share: the kernel arguments, the layout of the per-layer constants in LDS, the launch, and the stages whose
// arithmetic does not depend on the MFMA operand type.  Those stages are written once so that the init embedding and the
// graph context of the two kernels stay bit-identical ("16-bit encoder").
//
// A stage reaches the fp32 copy of h in LDS through the kernel's layout type Lay (passed by value, like every argument of
// the stages: see FusedArgs):
//   Lay::S                  row stride: element (row, c) is at col(c)[row * S]
//   col(c)                  the float* of column c in row 0
//   store4(row, q4, v)      columns 4 q4 .. 4 q4 + 3 of a row  <- v (and the 16-bit kernel's T copy)
//   load4(row, q4)          the same four values
//   mirror(row, c, y)       after col(c)[row * S] = y: keep the 16-bit kernel's T copy in step (fp32: nothing)
#pragma once
#include <type_traits>

#include "mfma_tile.hpp"      // f32x4, mf

namespace eamrl {

constexpr int FE = 128;          // embed dim
constexpr int FH = 8;            // heads
constexpr int FF = 512;          // feed-forward hidden
constexpr int MAX_FUSED_LAYERS = 8;
constexpr int NCST = 9 * FE + FF;     // floats of per-layer constants staged in LDS
// CST: bqkv [3E] | bo [E] | b1 [F] | b2 [E] | norm1 (scale | shift, or gamma | beta) [2E] | norm2 [2E]
constexpr int C_BQKV = 0, C_BO = 3 * FE, C_B1 = 4 * FE, C_B2 = 4 * FE + FF, C_N1 = 5 * FE + FF, C_N2 = 7 * FE + FF;

// The kernel argument.  The packed weights of L[] and cache.Wc / cache.WoutT are fp32 (pack_mfma_b) for k_encoder_fused and
// 16-bit (pack16) for k_encoder_fused16; everything else is fp32 for both.  The stages below take its fields by value, not
// a reference to it: a pointer into the argument handed to a helper keeps the argument in scratch until the helper is
// inlined, and the kernel then loses its scalar (uniform) loads -- other registers, other code (a reference to the kernel's
// layout object delays its promotion to registers the same way).  For the same reason each
// kernel stages its layer constants into CST itself, reading the layer's pointers where it uses them (k_encoder_fused:
// cst_request / cst_store, a phase apart; k_encoder_fused16: one loop at the layer top).
struct FusedArgs {
    const float* h_in; float* h_out; int M; int nlayers; int norm; float eps;
    eamrl_encoder_cache cache;   // cache.out null: no decoder cache; cache.gctx null: no graph context
    eamrl_encoder_init init;     // used when h_in is null
    eamrl_encoder_layer L[MAX_FUSED_LAYERS];
};

// ---- host ------------------------------------------------------------------------------------------------------------------

// encoder_fused16.hip: k_encoder_fused16<T> for dtype EAMRL_DTYPE_F16 / EAMRL_DTYPE_BF16
int launch_encoder_fused16(const FusedArgs& a, int64_t B, int dtype, hipStream_t st);

struct FusedVariant {
    void (*kernel)(FusedArgs);
    size_t lds;                  // dynamic LDS bytes
};

// One workgroup of 512 threads per instance.  The kernels come in three variants by the number RTT of 16-row tiles that
// hold the M nodes; variant(std::integral_constant<int, RTT>) returns the kernel of that RTT and its LDS bytes.
template <typename Variant>
int launch_fused(const FusedArgs& a, int64_t B, hipStream_t st, Variant variant)
{
    const FusedVariant v = a.M <= 32 ? variant(std::integral_constant<int, 2>())
                         : a.M <= 64 ? variant(std::integral_constant<int, 4>())
                                     : variant(std::integral_constant<int, 7>());
    if (v.lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(v.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds) !=
            hipSuccess)
        return EAMRL_E_LAUNCH;
    hipLaunchKernelGGL(v.kernel, dim3((unsigned)B), dim3(512), v.lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

// ---- device stages ---------------------------------------------------------------------------------------------------------

// h_in (row-major, HBM) into LDS; rows M .. ROWS-1 are zero.  All of a thread's loads are issued before the first LDS store
// (a load-store loop pays the HBM latency once per trip: 7 trips = 27 k of the kernel's 900 k cycles,
// profiles/r03b_stamps_encoder_fused.txt).
template <int ROWS, typename Lay>
__device__ __forceinline__ void load_h(const float* h_in, int M, const Lay L)
{
    const int tid = threadIdx.x;
    constexpr int NLD = (ROWS * (FE / 4) + 511) / 512;
    const float* src = h_in + (int64_t)blockIdx.x * (int64_t)M * FE;
    float4 v[NLD];
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
        const int idx = tid + u * 512;
        const int row = idx / (FE / 4), q4 = idx % (FE / 4);
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < M) v[u] = *reinterpret_cast<const float4*>(src + (int64_t)row * FE + 4 * q4);
    }
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
        const int idx = tid + u * 512;
        const int row = idx / (FE / 4), q4 = idx % (FE / 4);
        if (row < ROWS) L.store4(row, q4, v[u]);
    }
}

// The init embedding computed into LDS (nn/env_embeddings/init.py: Linear(F -> E) of the node features; depot envs: row 0
// is Linear(2 -> E) of the depot coordinates): each output is chain_k(x[k], W[c][k], F, bias[c]), the order of
// eamrl_linear.  Thread = (row, four adjacent columns); the weights of its columns stay in registers over the rows.
// Like load_h, a thread issues ALL its loads -- weights, biases, the depot coordinates and the features of every row trip --
// before the first wait, and none of them sits under a branch: an index past F or M is clamped (the value is then not
// used; so is row 0 of feat in a depot env), an absent pointer is replaced by W at index 0.  The init_out stores follow the
// LDS stores.
// KM: the number of feature loads per row, F <= KM (init_embedding dispatches once on F).
template <int ROWS, int KM, typename Lay>
__device__ __forceinline__ void init_embedding_f(const eamrl_encoder_init in, int M, const Lay L)
{
    constexpr int NT = ROWS / 16;
    const int tid = threadIdx.x;
    const int64_t inst = blockIdx.x;
    const int q4 = tid % (FE / 4), r0 = tid / (FE / 4);          // 32 column groups x 16 row phases
    const int F = in.F;
    const bool has_depot = in.depot != nullptr;
    const float* bp = in.b ? in.b : in.W;
    const float* bdp = (has_depot && in.bd) ? in.bd : in.W;
    const float* wdp = has_depot ? in.Wd : in.W;
    const float* dp = has_depot ? in.depot + inst * in.depot_ld : in.W;
    const int bm = in.b ? 1 : 0, bdm = (has_depot && in.bd) ? 1 : 0, dm = has_depot ? 1 : 0;
    float w[4][KM], wd[4][2], bb[4], bdv[4], x[NT][KM];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        bb[c] = bp[(4 * q4 + c) * bm];
        bdv[c] = bdp[(4 * q4 + c) * bdm];
#pragma unroll
        for (int k = 0; k < KM; ++k) w[c][k] = in.W[(4 * q4 + c) * F + (k < F ? k : F - 1)];
#pragma unroll
        for (int k = 0; k < 2; ++k) wd[c][k] = wdp[((4 * q4 + c) * 2 + k) * dm];
    }
    const float x0 = dp[0], x1 = dp[dm];
    const float* fsrc = in.feat + inst * (int64_t)M * F;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int row = r0 + 16 * t;
        const float* fr = fsrc + (int64_t)(row < M ? row : M - 1) * F;
#pragma unroll
        for (int k = 0; k < KM; ++k) x[t][k] = fr[k < F ? k : F - 1];
    }
    __builtin_amdgcn_sched_barrier(0);         // (left alone, the scheduler sinks the later rows' loads behind the first rows' waits)
    float y[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int row = r0 + 16 * t;
        const bool drow = has_depot && row == 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float acc = bm ? bb[c] : 0.0f;
#pragma unroll
            for (int k = 0; k < KM; ++k) acc = (k < F) ? fma_(x[t][k], w[c][k], acc) : acc;
            const float yd = fma_(x1, wd[c][1], fma_(x0, wd[c][0], bdm ? bdv[c] : 0.0f));
            y[t][c] = row < M ? (drow ? yd : acc) : 0.0f;
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) L.store4(r0 + 16 * t, q4, make_float4(y[t][0], y[t][1], y[t][2], y[t][3]));
    if (in.init_out) {
        float* iout = in.init_out + inst * (int64_t)M * FE;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int row = r0 + 16 * t;
            if (row < M) *reinterpret_cast<float4*>(iout + (int64_t)row * FE + 4 * q4) = make_float4(y[t][0], y[t][1], y[t][2], y[t][3]);
        }
    }
}

template <int ROWS, typename Lay>
__device__ __forceinline__ void init_embedding(const eamrl_encoder_init in, int M, const Lay L)
{
    if (in.F <= 2) init_embedding_f<ROWS, 2>(in, M, L);
    else if (in.F <= 4) init_embedding_f<ROWS, 4>(in, M, L);
    else init_embedding_f<ROWS, 8>(in, M, L);
}

// InstanceNorm1d(affine) in place: thread = channel, sequential over the M nodes (the order of k_norm_instance)
template <typename Lay>
__device__ __forceinline__ void instance_norm(const Lay L, int M, float eps, const float* cst /* LDS: gamma [E] | beta [E] */)
{
    const int c = threadIdx.x;
    if (c < FE) {
        float* col = L.col(c);
        float s = 0.0f;
        for (int n = 0; n < M; ++n) s = s + col[n * Lay::S];
        const float mean = s / (float)M;
        float v = 0.0f;
        for (int n = 0; n < M; ++n) { const float d = col[n * Lay::S] - mean; v = fma_(d, d, v); }
        const float inv = 1.0f / __builtin_sqrtf(v / (float)M + eps);
        const float g = cst[c], bt = cst[FE + c];
        for (int n = 0; n < M; ++n) {
            const float y = fma_((col[n * Lay::S] - mean) * inv, g, bt);
            col[n * Lay::S] = y;
            L.mirror(n, c, y);
        }
    }
}

// h -> h_out (row-major, float4 per thread)
template <typename Lay>
__device__ __forceinline__ void store_h(float* h_out, int M, const Lay L)
{
    float* dst = h_out + (int64_t)blockIdx.x * (int64_t)M * FE;
    for (int idx = threadIdx.x; idx < M * (FE / 4); idx += blockDim.x) {
        const int row = idx / (FE / 4), q4 = idx % (FE / 4);
        *reinterpret_cast<float4*>(dst + (int64_t)row * FE + 4 * q4) = L.load4(row, q4);
    }
}

// Graph context: mean over the nodes in node order (k_mean_nodes), then a k-ordered chain per output (k_linear).
// MEAN: FE floats of LDS that are free now.
template <typename Lay>
__device__ __forceinline__ void graph_context(const float* Wg, float* gctx, int M, const Lay L, float* MEAN)
{
    const int tid = threadIdx.x;
    if (tid < FE) {
        const float* col = L.col(tid);
        float s = 0.0f;
        for (int n = 0; n < M; ++n) s = s + col[n * Lay::S];
        MEAN[tid] = s / (float)M;
    }
    __syncthreads();
    if (tid < FE) {
        const float4* w = reinterpret_cast<const float4*>(Wg + (int64_t)tid * FE);
        float acc = 0.0f;
#pragma unroll 8
        for (int k4 = 0; k4 < FE / 4; ++k4) {
            const float4 wv4 = w[k4];
            acc = fma_(MEAN[4 * k4 + 0], wv4.x, acc);
            acc = fma_(MEAN[4 * k4 + 1], wv4.y, acc);
            acc = fma_(MEAN[4 * k4 + 2], wv4.z, acc);
            acc = fma_(MEAN[4 * k4 + 3], wv4.w, acc);
        }
        gctx[(int64_t)blockIdx.x * FE + tid] = acc;
    }
}

}  // namespace eamrl
