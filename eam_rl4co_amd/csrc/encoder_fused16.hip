// The fused per-instance encoder of encoder_fused.hip with 16-bit MFMA operands (T = fp16 or bf16): the same phase plan
// (one workgroup per instance, all layers, the optional init embedding in front and the decoder cache behind), every Linear
// on v_mfma_f32_16x16x32_{f16,bf16} and the attention scores / value products on v_mfma_f32_16x16x16_{f16,bf16}.
//
// Reference: rl4co/models/nn/graph/attnnet.py:16-103 (MultiHeadAttentionLayer / GraphAttentionNetwork),
// rl4co/models/nn/attention.py:66-136 (MultiHeadAttention), rl4co/models/nn/ops.py:32-56 (Normalization),
// rl4co/models/nn/mlp.py:52-61 (MLP 128 -> 512 -> 128, ReLU), rl4co/models/zoo/am/decoder.py:206-235 (the cache).
//
// Arithmetic = the 16-bit contract of DESIGN.md 2 ("Rounded to T" = round-to-nearest-even of the fp32 value):
//   * node Linears: both operands rounded to T, products and sums accumulated in fp32 by the MFMA, the fp32 bias is the
//     accumulator's initial value, the output is fp32;
//   * attention: q * 0.25, k, v rounded to T; scores accumulated in fp32; max, d_expf and the softmax in fp32; the weights w
//     rounded to T for the value product; Z = fp32 sum of the rounded weights; o = (sum w v) / Z in fp32;
//   * residual adds, BatchNorm (eval), InstanceNorm, ReLU in fp32 (the residual stream HB stays fp32 in LDS); a T copy HT of
//     h is what the next Linear reads;
//   * h load / store, init embedding, InstanceNorm and graph context: the shared stages of encoder_fused.hpp (load_h,
//     init_embedding, store_h, instance_norm, graph_context) that k_encoder_fused runs too, so the init embeddings are
//     bit-identical to it.
// There is no bit-exact oracle: the accumulation order inside a 16-bit MFMA is not documented.
//
// Every GEMM pass is "swapped": the packed weight fragment is the MFMA's A operand and the activation fragment its B operand,
// so that lane (j = lane & 15, G = lane >> 4) of accumulator tile (rt, ct) holds node row 16 rt + j and the four consecutive
// output columns 16 ct + 4 G + (0..3): one float4 / 8-byte store per tile, biases as float4 reads.
//
// LDS (ROWS = 16 RTT rows; strides in elements):
//   HB  fp32 [ROWS][SH]  residual stream          HT  T [ROWS][ST]  h rounded to T (A operand of Wqkv, W1, the cache)
//   QA  T [ROWS][SQ]     q * 0.25 of the head group, then the attention output     KB  T [ROWS][SQ]  k of the head group
//   VT  T [64][SV]       v of the head group, transposed (keys contiguous)         HID T [ROWS][ST]  aliases QA | KB | VT
//   CST fp32             the layer's biases and normalisation constants
// Row strides of 272 B (HT, HID) and 144 B (QA, KB) put the 16 rows of a ds_read_b128 fragment on distinct bank quads.
#include "encoder_fused.hpp"

namespace eamrl {
namespace {

constexpr int SH = 132;          // HB row stride (floats)
constexpr int ST = 136;          // HT / HID row stride (T)
constexpr int SQ = 72;           // QA / KB row stride (T)

// T-specific fragment types and MFMA builtins
template <typename T> struct Mf;
template <> struct Mf<__bf16> {
    typedef __bf16 v8 __attribute__((ext_vector_type(8)));
    typedef __bf16 v4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ f32x4 k32(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 k16(v4 a, v4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0); }
};
template <> struct Mf<_Float16> {
    typedef _Float16 v8 __attribute__((ext_vector_type(8)));
    typedef _Float16 v4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ f32x4 k32(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 k16(v4 a, v4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
};

// four fp32 -> four T, round to nearest even (v_cvt_pk_*), stored as 8 bytes
template <typename T>
__device__ __forceinline__ typename Mf<T>::v4 cvt4(float a, float b, float c, float d)
{
    return (typename Mf<T>::v4){(T)a, (T)b, (T)c, (T)d};
}

// h: fp32 HB and its T copy HT, both row-major, for the shared stages of encoder_fused.hpp
template <typename T>
struct Layout16 {
    float* HB; T* HT;
    static constexpr int S = SH;
    __device__ float* col(int c) const { return HB + c; }
    __device__ void store4(int row, int q4, float4 v) const
    {
        *reinterpret_cast<float4*>(HB + row * SH + 4 * q4) = v;
        *reinterpret_cast<typename Mf<T>::v4*>(HT + row * ST + 4 * q4) = cvt4<T>(v.x, v.y, v.z, v.w);
    }
    __device__ float4 load4(int row, int q4) const { return *reinterpret_cast<const float4*>(HB + row * SH + 4 * q4); }
    __device__ void mirror(int row, int c, float y) const { HT[row * ST + c] = (T)y; }
};

// acc[rt][ct] += W[16 ct' + i][k] * A[row 16 rt + j][k] over NU k-groups of 32.
//   arow: this lane's activation fragment of tile 0, group 0 (LDS: row row0 + j, column 8 G), tiles 16 S elements apart
//   wp[ct]: this lane's weight fragment of group 0 (consecutive groups 64 fragments apart)
template <typename T, int RTW, int CT, int NU, int NRT>
__device__ __forceinline__ void gemm16_n(f32x4 (&acc)[RTW][CT], const T* arow, int S, const typename Mf<T>::v8* const (&wp)[CT])
{
    typedef typename Mf<T>::v8 v8;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        v8 b[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) b[ct] = wp[ct][u * 64];
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
            const v8 a = *reinterpret_cast<const v8*>(arow + rt * 16 * S + 32 * u);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = Mf<T>::k32(b[ct], a, acc[rt][ct]);
        }
    }
}

template <typename T, int RTW, int CT, int NU, int NLOW>
__device__ __forceinline__ void gemm16(f32x4 (&acc)[RTW][CT], const T* arow, int S, int nrt, const typename Mf<T>::v8* const (&wp)[CT])
{
    if (NLOW == RTW || nrt == RTW) gemm16_n<T, RTW, CT, NU, RTW>(acc, arow, S, wp);
    else gemm16_n<T, RTW, CT, NU, NLOW>(acc, arow, S, wp);
}

// this lane's fragment of group 0 of column tile ct of a packed weight with K inputs
template <typename T>
__device__ __forceinline__ const typename Mf<T>::v8* wfrag(const void* Wp, int ct, int K, int u0, int lane)
{
    return reinterpret_cast<const typename Mf<T>::v8*>(Wp) + ((int64_t)ct * (K / 32) + u0) * 64 + lane;
}

// h = norm(h + acc) on the wave's tiles (HB in place); the T copy HT is written here for batch norm (instance norm: after
// the per-channel pass)
template <typename T, int RTW>
__device__ __forceinline__ void residual_norm16(const f32x4 (&acc)[RTW][2], float* HB, T* HT, int row0, int nrt, int cw, int j,
                                                int G, int norm, const float* cst)
{
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int c = 32 * cw + 16 * ct + 4 * G;
        const float4 sc = *reinterpret_cast<const float4*>(cst + c), sh = *reinterpret_cast<const float4*>(cst + FE + c);
#pragma unroll
        for (int rt = 0; rt < RTW; ++rt)
            if (rt < nrt) {
                const int row = row0 + 16 * rt + j;
                float4* p = reinterpret_cast<float4*>(HB + row * SH + c);
                float4 v = *p;
                v.x = v.x + acc[rt][ct][0]; v.y = v.y + acc[rt][ct][1]; v.z = v.z + acc[rt][ct][2]; v.w = v.w + acc[rt][ct][3];
                if (norm == EAMRL_NORM_BATCH_EVAL) {
                    v.x = fma_(v.x, sc.x, sh.x); v.y = fma_(v.y, sc.y, sh.y); v.z = fma_(v.z, sc.z, sh.z); v.w = fma_(v.w, sc.w, sh.w);
                    *reinterpret_cast<typename Mf<T>::v4*>(HT + row * ST + c) = cvt4<T>(v.x, v.y, v.z, v.w);
                }
                *p = v;
            }
    }
}

template <typename T, int RTT>
__global__ __launch_bounds__(512, 1) void k_encoder_fused16(FusedArgs a)
{
    typedef typename Mf<T>::v8 v8;
    typedef typename Mf<T>::v4 v4;
    constexpr int RTA = (RTT + 1) / 2;
    constexpr int RTW = RTA;
    constexpr int ROWS = 16 * RTT;
    constexpr int SV = ROWS + 8;                // VT row stride (T)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* HB = lds;                                            // [ROWS][SH] fp32
    float* CST = HB + ROWS * SH;                                // [NCST] fp32
    T* HT = reinterpret_cast<T*>(CST + NCST);                   // [ROWS][ST]
    T* QA = HT + ROWS * ST;                                     // [ROWS][SQ]
    T* KB = QA + ROWS * SQ;                                     // [ROWS][SQ]
    T* VT = KB + ROWS * SQ;                                     // [64][SV]
    T* HID = QA;                                                // [ROWS][ST]
    static_assert(ROWS * ST <= 2 * ROWS * SQ + 64 * SV, "HID must fit QA | KB | VT");
    const Layout16<T> L{HB, HT};

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cw = wv & 3, rw = wv >> 2;
    const int j = lane & 15, G = lane >> 4;
    const int M = a.M;
    const int row0 = rw ? 16 * RTA : 0;
    const int nrt = rw ? RTT - RTA : RTA;
    const int64_t inst = blockIdx.x;

    // ---- h into HB (fp32) and HT (T); rows >= M are zero --------------------------------------------------------------
    if (a.h_in) load_h<ROWS>(a.h_in, M, L);
    else init_embedding<ROWS>(a.init, M, L);
    __syncthreads();

    for (int layer = 0; layer < a.nlayers; ++layer) {
        const eamrl_encoder_layer& Ly = a.L[layer];
        for (int i = tid; i < NCST; i += blockDim.x) {
            float v;
            if (i < C_BO) v = Ly.bqkv[i];
            else if (i < C_B1) v = Ly.bo[i - C_BO];
            else if (i < C_B2) v = Ly.b1[i - C_B1];
            else if (i < C_N1) v = Ly.b2[i - C_B2];
            else {
                const bool second = i >= C_N2;
                const int k = (i - (second ? C_N2 : C_N1));
                const int c = k & (FE - 1);
                const float* gam = second ? Ly.n2_gamma : Ly.n1_gamma;
                const float* bet = second ? Ly.n2_beta : Ly.n1_beta;
                if (a.norm == EAMRL_NORM_BATCH_EVAL) {
                    const float* mean = second ? Ly.n2_mean : Ly.n1_mean;
                    const float* var = second ? Ly.n2_var : Ly.n1_var;
                    const float sc = gam[c] / __builtin_sqrtf(var[c] + a.eps);
                    const float ms = mean[c] * sc;
                    v = k < FE ? sc : bet[c] - ms;
                } else {
                    v = k < FE ? gam[c] : bet[c];
                }
            }
            CST[i] = v;
        }
        __syncthreads();
        f32x4 acc_o[RTW][2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const float4 b = *reinterpret_cast<const float4*>(CST + C_BO + 32 * cw + 16 * ct + 4 * G);
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) acc_o[rt][ct] = (f32x4){b.x, b.y, b.z, b.w};
        }
        for (int hg = 0; hg < 2; ++hg) {
            // ---- P1: q | k | v of head 4 hg + cw --------------------------------------------------------------------------
            {
                f32x4 acc[RTW][3];
                const int ctq = 4 * hg + cw;
                const v8* wp[3];
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    wp[x] = wfrag<T>(Ly.Wqkv, 8 * x + ctq, FE, 0, lane);
                    const float4 b = *reinterpret_cast<const float4*>(CST + C_BQKV + 16 * (8 * x + ctq) + 4 * G);
#pragma unroll
                    for (int rt = 0; rt < RTW; ++rt) acc[rt][x] = (f32x4){b.x, b.y, b.z, b.w};
                }
                gemm16<T, RTW, 3, FE / 32, RTT - RTA>(acc, HT + (row0 + j) * ST + 8 * G, ST, nrt, wp);
#pragma unroll
                for (int rt = 0; rt < RTW; ++rt)
                    if (rt < nrt) {
                        const int row = row0 + 16 * rt + j;
                        const int d = 16 * cw + 4 * G;          // head-group column of register 0
                        *reinterpret_cast<v4*>(QA + row * SQ + d) =
                            cvt4<T>(acc[rt][0][0] * 0.25f, acc[rt][0][1] * 0.25f, acc[rt][0][2] * 0.25f, acc[rt][0][3] * 0.25f);
                        *reinterpret_cast<v4*>(KB + row * SQ + d) = cvt4<T>(acc[rt][1][0], acc[rt][1][1], acc[rt][1][2], acc[rt][1][3]);
#pragma unroll
                        for (int r = 0; r < 4; ++r) VT[(d + r) * SV + row] = (T)acc[rt][2][r];
                    }
            }
            __syncthreads();
            // ---- P2: attention of head cw of the group, the query tiles of this wave half ---------------------------------
            {
                // scores S^T = K Q^T (keys on MFMA rows, in order): lane (query j, G), register r = key 16 kt + 4 G + r, which
                // is also the B operand layout (k = 4 G + r) of the 16x16x16 value product of key tile kt
                v4 kf[RTT], vf[RTT];
#pragma unroll
                for (int kt = 0; kt < RTT; ++kt) {
                    kf[kt] = *reinterpret_cast<const v4*>(KB + (16 * kt + j) * SQ + 16 * cw + 4 * G);
                    vf[kt] = *reinterpret_cast<const v4*>(VT + (16 * cw + j) * SV + 16 * kt + 4 * G);
#pragma unroll
                    for (int r = 0; r < 4; ++r)         // padded keys: zero values (rows >= M of h are not normalised)
                        if (16 * kt + 4 * G + r >= M) vf[kt][r] = (T)0.0f;
                }
                for (int q = 0; q < nrt; ++q) {
                    const int qrow = row0 + 16 * q + j;
                    const v4 qf = *reinterpret_cast<const v4*>(QA + qrow * SQ + 16 * cw + 4 * G);
                    f32x4 s[RTT];
                    float m = -INFINITY;
#pragma unroll
                    for (int kt = 0; kt < RTT; ++kt) s[kt] = Mf<T>::k16(kf[kt], qf, splat4(0.0f));
#pragma unroll
                    for (int kt = 0; kt < RTT; ++kt) {
                        if (16 * kt + 16 > M) {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (16 * kt + 4 * G + r >= M) s[kt][r] = -INFINITY;
                        }
                        m = vmax5_raw(m, s[kt][0], s[kt][1], s[kt][2], s[kt][3]);
                    }
                    {
                        auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
                        m = vmax_raw(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
                        auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
                        m = vmax_raw(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
                    }
                    v4 wt[RTT];
                    float zp = 0.0f;
#pragma unroll
                    for (int kt = 0; kt < RTT; ++kt) {
                        f32x2 e01 = (f32x2){s[kt][0], s[kt][1]} - splat2(m), e23 = (f32x2){s[kt][2], s[kt][3]} - splat2(m);
                        d_expf2_nonpos_x2(e01, e23);
                        wt[kt] = cvt4<T>(e01.x, e01.y, e23.x, e23.y);
#pragma unroll
                        for (int r = 0; r < 4; ++r) zp = zp + (float)wt[kt][r];
                    }
                    {
                        auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(zp), __float_as_uint(zp), false, false);
                        zp = __uint_as_float(r16[0]) + __uint_as_float(r16[1]);
                        auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(zp), __float_as_uint(zp), false, false);
                        zp = __uint_as_float(r32[0]) + __uint_as_float(r32[1]);
                    }
                    // o^T = V^T W: lane (query j, G), register r = head column 4 G + r
                    f32x4 o = splat4(0.0f);
#pragma unroll
                    for (int kt = 0; kt < RTT; ++kt)
                        if (16 * kt < M) o = Mf<T>::k16(vf[kt], wt[kt], o);
                    *reinterpret_cast<v4*>(QA + qrow * SQ + 16 * cw + 4 * G) = cvt4<T>(o[0] / zp, o[1] / zp, o[2] / zp, o[3] / zp);
                }
            }
            __syncthreads();
            // ---- P3: out_proj partial over the 64 attention columns of this head group ------------------------------------
            {
                const v8* wp3[2];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) wp3[ct] = wfrag<T>(Ly.Wo, 2 * cw + ct, FE, 2 * hg, lane);
                gemm16<T, RTW, 2, 2, RTT - RTA>(acc_o, QA + (row0 + j) * SQ + 8 * G, SQ, nrt, wp3);
            }
            __syncthreads();
        }
        // ---- h1 = norm1(h + out_proj) ---------------------------------------------------------------------------------------
        residual_norm16<T, RTW>(acc_o, HB, HT, row0, nrt, cw, j, G, a.norm, CST + C_N1);
        __syncthreads();
        if (a.norm == EAMRL_NORM_INSTANCE) {
            instance_norm(L, M, a.eps, CST + C_N1);
            __syncthreads();
        }
        // ---- FFN: 4 chunks of 128 hidden units ---------------------------------------------------------------------------
        f32x4 acc_f[RTW][2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const float4 b = *reinterpret_cast<const float4*>(CST + C_B2 + 32 * cw + 16 * ct + 4 * G);
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) acc_f[rt][ct] = (f32x4){b.x, b.y, b.z, b.w};
        }
        for (int ch = 0; ch < FF / 128; ++ch) {
            {   // P4: hidden chunk = relu(h1 W1_ch^T + b1) -> HID (T)
                f32x4 acc[RTW][2];
                const v8* wp[2];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const int ctile = 8 * ch + 2 * cw + ct;
                    wp[ct] = wfrag<T>(Ly.W1, ctile, FE, 0, lane);
                    const float4 b = *reinterpret_cast<const float4*>(CST + C_B1 + 16 * ctile + 4 * G);
#pragma unroll
                    for (int rt = 0; rt < RTW; ++rt) acc[rt][ct] = (f32x4){b.x, b.y, b.z, b.w};
                }
                gemm16<T, RTW, 2, FE / 32, RTT - RTA>(acc, HT + (row0 + j) * ST + 8 * G, ST, nrt, wp);
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int rt = 0; rt < RTW; ++rt)
                        if (rt < nrt) {
                            float y[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) { const float v = acc[rt][ct][r]; y[r] = !(v > 0.0f) ? 0.0f : v; }
                            *reinterpret_cast<v4*>(HID + (row0 + 16 * rt + j) * ST + 32 * cw + 16 * ct + 4 * G) =
                                cvt4<T>(y[0], y[1], y[2], y[3]);
                        }
            }
            __syncthreads();
            {   // P5: ffn2 accumulators += hidden chunk x W2[:, 128 ch .. 128 ch + 127]^T
                const v8* wp5[2];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) wp5[ct] = wfrag<T>(Ly.W2, 2 * cw + ct, FF, 4 * ch, lane);
                gemm16<T, RTW, 2, 4, RTT - RTA>(acc_f, HID + (row0 + j) * ST + 8 * G, ST, nrt, wp5);
            }
            __syncthreads();
        }
        // ---- h2 = norm2(h1 + ffn) ------------------------------------------------------------------------------------------
        residual_norm16<T, RTW>(acc_f, HB, HT, row0, nrt, cw, j, G, a.norm, CST + C_N2);
        __syncthreads();
        if (a.norm == EAMRL_NORM_INSTANCE) {
            instance_norm(L, M, a.eps, CST + C_N2);
            __syncthreads();
        }
    }
    // ---- embeddings out (fp32, row-major), graph context ---------------------------------------------------------------------
    if (a.h_out) store_h(a.h_out, M, L);
    if (a.cache.gctx) graph_context(a.cache.Wg, a.cache.gctx, M, L, CST);
    // ---- decoder cache: nproj projections of h, then Lp = L Wout (L rounded to T in STG) ------------------------------------
    if (a.cache.out) {
        T* STG = QA;                                // [ROWS][ST], aliases the dead attention / hidden buffers
        float* crow = a.cache.out + (inst * (int64_t)M) * a.cache.ld;
        for (int sl = 0; sl <= a.cache.nproj; ++sl) {
            const bool lp = sl == a.cache.nproj;
            f32x4 acc[RTW][2];
            const v8* wp[2];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                wp[ct] = lp ? wfrag<T>(a.cache.WoutT, 2 * cw + ct, FE, 0, lane) : wfrag<T>(a.cache.Wc, 8 * sl + 2 * cw + ct, FE, 0, lane);
#pragma unroll
                for (int rt = 0; rt < RTW; ++rt) acc[rt][ct] = splat4(0.0f);
            }
            if (lp) __syncthreads();
            gemm16<T, RTW, 2, FE / 32, RTT - RTA>(acc, (lp ? STG : HT) + (row0 + j) * ST + 8 * G, ST, nrt, wp);
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt)
                if (rt < nrt) {
                    const int node = row0 + 16 * rt + j;
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        const int c = 32 * cw + 16 * ct + 4 * G;
                        const f32x4 v = acc[rt][ct];
                        if (node < M)
                            *reinterpret_cast<float4*>(crow + (int64_t)node * a.cache.ld + sl * FE + c) = make_float4(v[0], v[1], v[2], v[3]);
                        if (sl == 2) *reinterpret_cast<v4*>(STG + node * ST + c) = cvt4<T>(v[0], v[1], v[2], v[3]);
                    }
                }
        }
    }
}

// Wp[ct][u][l][e] = T(W[16 ct + (l & 15)][32 u + 8 (l >> 4) + e]): lane l of a 16x16x32 MFMA finds its 8 operand values
// of k-group u in 16 contiguous bytes, and a wavefront's 64 fragments are 1 KB contiguous.
template <typename T>
__global__ void k_pack16(const float* __restrict__ W, T* __restrict__ Wp, int N, int K)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)N * K) return;
    const int e = (int)(idx & 7), l = (int)((idx >> 3) & 63);
    const int64_t blk = idx >> 9;                 // ct * (K / 32) + u
    const int u = (int)(blk % (K / 32)), ct = (int)(blk / (K / 32));
    Wp[idx] = (T)W[(int64_t)(16 * ct + (l & 15)) * K + 32 * u + 8 * (l >> 4) + e];
}

template <typename T>
int launch16(const FusedArgs& a, int64_t B, hipStream_t st)
{
    return launch_fused(a, B, st, [](auto rtt) {
        constexpr int RTT = decltype(rtt)::value, ROWS = 16 * RTT;
        return FusedVariant{k_encoder_fused16<T, RTT>, ((size_t)ROWS * SH + NCST) * sizeof(float) +
                                                           ((size_t)ROWS * ST + 2 * (size_t)ROWS * SQ + 64 * (size_t)(ROWS + 8)) * sizeof(T)};
    });
}

}  // namespace

int launch_pack_mfma_b16(const float* W, void* Wp, int N, int K, int dtype, hipStream_t st)
{
    const int64_t n = (int64_t)N * K;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == EAMRL_DTYPE_BF16) hipLaunchKernelGGL(k_pack16<__bf16>, grid, dim3(256), 0, st, W, (__bf16*)Wp, N, K);
    else hipLaunchKernelGGL(k_pack16<_Float16>, grid, dim3(256), 0, st, W, (_Float16*)Wp, N, K);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

int launch_encoder_fused16(const FusedArgs& a, int64_t B, int dtype, hipStream_t st)
{
    return dtype == EAMRL_DTYPE_BF16 ? launch16<__bf16>(a, B, st) : launch16<_Float16>(a, B, st);
}

}  // namespace eamrl
