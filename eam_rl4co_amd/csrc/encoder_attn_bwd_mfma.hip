// Encoder self-attention backward for graphs of 113 to 1024 nodes on fp32 MFMA (k_mha_encoder_bwd keeps a whole instance in one
// workgroup and stops at 112 nodes).  Same interface: qkv [B][N][3E] packed "b s (three h d)" as given to the forward,
// dO [B][N][E] -> dqkv [B][N][3E] (written).  E = 128, H = 8, D = 16, the scale 1/4 folded into q (q~ = q / 4):
//   S = q~ K^T,  P = softmax_rows(S),  dP = dO V^T,  Delta = rowsum(P o dP) (= rowsum(dO o O): nothing from the forward is kept),
//   dS = P o (dP - Delta),  dV = P^T dO,  dK = dS^T q~,  dq = 0.25 dS K.
//
// One workgroup = (instance, head), 8 wavefronts.  The head's keys and values are staged once in LDS as the B operands of the two
// "sum over d" products -- per 16-key tile kt and lane (j, G): KB[kt][lane] = K[16 kt + j][4 G .. 4 G + 3], VB likewise -- so the
// score and dP tiles come out with the query on the accumulator row (register r of lane group G: query 4 G + r) and the key on
// the lane (j).  In that orientation P and dS are, as they stand, the B operands of the two "sum over queries" products dV^T and
// dK^T; only dq (a sum over keys) needs dS transposed, through a 16 x 16 tile of the wave's own in LDS.
// Wave w owns the key tiles kt = w, w + 8, ... (at most U = 8) and keeps their dK / dV accumulators, scores and dP in registers
// (the K^T fragments of the dq product are read from KB).  All waves walk the query tiles together; per query tile:
//   phase 1  S and dP of the wave's tiles; per query the wave's max m_w over its keys, Z_w = sum exp(S - m_w) and
//            X_w = sum exp(S - m_w) dP
//            (lane partials in ascending tile order, then a fixed butterfly over the 16 lanes of a row); (m_w, Z_w, X_w) -> LDS;
//   barrier
//   phase 2  every wave combines the 8 partials in wave order: m = max m_w, Z = sum Z_w exp(m_w - m), X likewise, Delta = X / Z;
//            P = exp(S - m_w) exp(m_w - m) / Z, dS, dV += P^T dO, dK += dS^T q~, the wave's dq partial -> LDS (double-buffered);
//            after the NEXT tile's barrier 256 threads add the 8 partials in wave order and store dq.
// One barrier per query tile, no atomics, and every sum has a fixed order: the result is deterministic and does not depend on the
// batch.  Keys >= N get -inf scores (P = dS = 0) and zero values; query rows >= N have zero q and dO and are not stored.
#include "mfma_tile.hpp"

namespace eamrl {

namespace {

constexpr int AE = 128, AH = 8, AD = 16;
constexpr int TRS = 20;                                 // row stride (floats) of the per-wave transpose tile

__device__ __forceinline__ void exp4_nonpos(f32x4& x)
{
    const f32x2 a = d_expf2_nonpos((f32x2){x[0], x[1]}), b = d_expf2_nonpos((f32x2){x[2], x[3]});
    x = (f32x4){a.x, a.y, b.x, b.y};
}

size_t bwd_lds_bytes(int N)
{
    const int NT = (N + 15) >> 4;
    return ((size_t)NT * 512 + 2 * 8 * 48 + 2 * 8 * 256 + 8 * 16 * TRS) * sizeof(float);
}

template <int U>
__global__ __launch_bounds__(512, 1) void k_mha_encoder_bwd_mfma(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                 float* __restrict__ dqkv, int N)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int NT = (N + 15) >> 4;
    float* KB = lds;                                    // [NT][64][4]
    float* VB = KB + (size_t)NT * 256;                  // [NT][64][4]
    float* STAT = VB + (size_t)NT * 256;                // [2][8 waves][m | Z | X][16 queries]
    float* DQP = STAT + 2 * 8 * 48;                     // [2][8 waves][4 registers][64 lanes]
    float* TR = DQP + 2 * 8 * 256;                      // [8 waves][16 queries][TRS]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, G = lane >> 4;
    const int64_t b = blockIdx.x / AH;
    const int h = (int)(blockIdx.x - b * AH);
    const float* qb = qkv + b * (int64_t)N * 3 * AE + h * AD;
    const float* ob = dout + b * (int64_t)N * AE + h * AD;
    float* gb = dqkv + b * (int64_t)N * 3 * AE + h * AD;

    // ---- stage K and V of this head (thread = key; keys beyond N are zeros) ------------------------------------------------------
    for (int n = tid; n < NT * 16; n += blockDim.x) {
        const int kt = n >> 4, kj = n & 15;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float4 kk = make_float4(0.f, 0.f, 0.f, 0.f), vv = kk;
            if (n < N) {
                kk = *reinterpret_cast<const float4*>(qb + (int64_t)n * 3 * AE + AE + 4 * g);
                vv = *reinterpret_cast<const float4*>(qb + (int64_t)n * 3 * AE + 2 * AE + 4 * g);
            }
            *reinterpret_cast<float4*>(KB + ((size_t)kt * 64 + 16 * g + kj) * 4) = kk;
            *reinterpret_cast<float4*>(VB + ((size_t)kt * 64 + 16 * g + kj) * 4) = vv;
        }
    }
    // ---- dK / dV accumulators of the wave's key tiles -------------------------------------------------------------------------
    f32x4 dV[U], dK[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        dV[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        dK[u] = dV[u];
    }
    // query rows of a tile as A operands of the "sum over d" products: lane (query j, G), k-step s -> d = 4 G + s
    auto fetch_rows = [&](int qt, float4& qa, float4& da) {
        const int n = 16 * qt + j;
        const int nc = n < N ? n : N - 1;
        qa = *reinterpret_cast<const float4*>(qb + (int64_t)nc * 3 * AE + 4 * G);
        da = *reinterpret_cast<const float4*>(ob + (int64_t)nc * AE + 4 * G);
        if (n >= N) { qa = make_float4(0.f, 0.f, 0.f, 0.f); da = qa; }
        qa.x *= 0.25f; qa.y *= 0.25f; qa.z *= 0.25f; qa.w *= 0.25f;
    };
    // dq of query tile qt: the 8 wave partials in wave order (256 threads, one element each)
    auto store_dq = [&](int qt) {
        if (tid < 256) {
            const float* p = DQP + (qt & 1) * 8 * 256 + tid;
            float acc = p[0];
#pragma unroll
            for (int w = 1; w < 8; ++w) acc = acc + p[w * 256];
            const int r = tid >> 6, ln = tid & 63;
            const int n = 16 * qt + 4 * (ln >> 4) + r;
            if (n < N) gb[(int64_t)n * 3 * AE + (ln & 15)] = 0.25f * acc;
        }
    };
    float4 qa_n, da_n;
    fetch_rows(0, qa_n, da_n);
    float* tr = TR + wv * 16 * TRS;
    __syncthreads();                                    // KB / VB

    for (int qt = 0; qt < NT; ++qt) {
        const int buf = qt & 1;
        const float4 qa = qa_n, da = da_n;
        if (qt + 1 < NT) fetch_rows(qt + 1, qa_n, da_n);
        // A operands of the "sum over queries" products: lane (d j, G), k-step s -> query 4 G + s
        float qc[4], dc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int n = 16 * qt + 4 * G + s;
            const int nc = n < N ? n : N - 1;
            const float qv = qb[(int64_t)nc * 3 * AE + j], dv = ob[(int64_t)nc * AE + j];
            qc[s] = n < N ? 0.25f * qv : 0.0f;
            dc[s] = n < N ? dv : 0.0f;
        }
        // ---- phase 1: scores and dP of the wave's key tiles, the wave's softmax partials --------------------------------------
        f32x4 sc[U], dp[U];
        f32x4 mw = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kt = wv + 8 * u;
            if (kt < NT) {                              // (uniform)
                const float4 kb = *reinterpret_cast<const float4*>(KB + ((size_t)kt * 64 + lane) * 4);
                const float4 vb = *reinterpret_cast<const float4*>(VB + ((size_t)kt * 64 + lane) * 4);
                f32x4 s = mf(qa.x, kb.x, (f32x4){0.f, 0.f, 0.f, 0.f});
                f32x4 d = mf(da.x, vb.x, (f32x4){0.f, 0.f, 0.f, 0.f});
                s = mf(qa.y, kb.y, s);
                d = mf(da.y, vb.y, d);
                s = mf(qa.z, kb.z, s);
                d = mf(da.z, vb.z, d);
                s = mf(qa.w, kb.w, s);
                d = mf(da.w, vb.w, d);
                if (16 * kt + j >= N) s = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                sc[u] = s;
                dp[u] = d;
#pragma unroll
                for (int r = 0; r < 4; ++r) mw[r] = fmaxf(mw[r], s[r]);
            }
        }
        f32x4 zw = (f32x4){0.f, 0.f, 0.f, 0.f}, xw = zw;
#pragma unroll
        for (int r = 0; r < 4; ++r) mw[r] = row_fmax_dpp(mw[r]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (wv + 8 * u < NT) {
                f32x4 e = sc[u] - mw;
                exp4_nonpos(e);
                sc[u] = e;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    zw[r] = zw[r] + e[r];
                    xw[r] = fmaf(e[r], dp[u][r], xw[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            zw[r] = row_sum_dpp(zw[r]);
            xw[r] = row_sum_dpp(xw[r]);
        }
        float* st = STAT + (buf * 8 + wv) * 48 + 4 * G;
        if (j == 0) {
            *reinterpret_cast<f32x4*>(st) = mw;
            *reinterpret_cast<f32x4*>(st + 16) = zw;
            *reinterpret_cast<f32x4*>(st + 32) = xw;
        }
        __syncthreads();
        if (qt > 0) store_dq(qt - 1);
        // ---- phase 2: combine the partials in wave order ------------------------------------------------------------------------
        const float* sp = STAT + buf * 8 * 48 + 4 * G;
        f32x4 m = *reinterpret_cast<const f32x4*>(sp);
#pragma unroll 2
        for (int w = 1; w < 8; ++w) {
            const f32x4 o = *reinterpret_cast<const f32x4*>(sp + w * 48);
#pragma unroll
            for (int r = 0; r < 4; ++r) m[r] = fmaxf(m[r], o[r]);
        }
        f32x4 Z = (f32x4){0.f, 0.f, 0.f, 0.f}, X = Z;
#pragma unroll 2
        for (int w = 0; w < 8; ++w) {
            f32x4 f = *reinterpret_cast<const f32x4*>(sp + w * 48) - m;
            exp4_nonpos(f);
            const f32x4 z = *reinterpret_cast<const f32x4*>(sp + w * 48 + 16), x = *reinterpret_cast<const f32x4*>(sp + w * 48 + 32);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Z[r] = fmaf(z[r], f[r], Z[r]);
                X[r] = fmaf(x[r], f[r], X[r]);
            }
        }
        f32x4 c = mw - m, delta;
        exp4_nonpos(c);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float iz = 1.0f / Z[r];
            c[r] = c[r] * iz;
            delta[r] = X[r] * iz;
        }
        // ---- phase 2: P, dS and the three products of the wave's key tiles ----------------------------------------------------
        f32x4 dq0 = (f32x4){0.f, 0.f, 0.f, 0.f}, dq1 = dq0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (wv + 8 * u < NT) {
                const f32x4 p = sc[u] * c;
                const f32x4 ds = p * (dp[u] - delta);
                dV[u] = mf(dc[0], p[0], dV[u]);
                dK[u] = mf(qc[0], ds[0], dK[u]);
                dV[u] = mf(dc[1], p[1], dV[u]);
                dK[u] = mf(qc[1], ds[1], dK[u]);
                dV[u] = mf(dc[2], p[2], dV[u]);
                dK[u] = mf(qc[2], ds[2], dK[u]);
                dV[u] = mf(dc[3], p[3], dV[u]);
                dK[u] = mf(qc[3], ds[3], dK[u]);
                // dS^T: element (query 4 G + r, key j) -> tr[query][key]; read back lane (query j, G): keys 4 G .. 4 G + 3
#pragma unroll
                for (int r = 0; r < 4; ++r) tr[(4 * G + r) * TRS + j] = ds[r];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const float4 a = *reinterpret_cast<const float4*>(tr + j * TRS + 4 * G);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                // B operand of dq: lane (d j, G), k-step s -> K[16 kt + 4 G + s][j] = KB[kt][lane 16 (j >> 2) + 4 G + s][j & 3]
                const float* kp = KB + ((size_t)(wv + 8 * u) * 64 + 16 * (j >> 2) + 4 * G) * 4 + (j & 3);
                f32x4& dq = (u & 1) ? dq1 : dq0;
                dq = mf(a.x, kp[0], dq);
                dq = mf(a.y, kp[4], dq);
                dq = mf(a.z, kp[8], dq);
                dq = mf(a.w, kp[12], dq);
            }
        }
        // dq partial: lane (d j, G), register r -> query 4 G + r
        const f32x4 dq = dq0 + dq1;
        float* dqp = DQP + (buf * 8 + wv) * 256 + lane;
#pragma unroll
        for (int r = 0; r < 4; ++r) dqp[r * 64] = dq[r];
    }
    __syncthreads();
    store_dq(NT - 1);
    // dV / dK: lane (key j, G), register r -> head column 4 G + r
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int n = 16 * (wv + 8 * u) + j;
        if (n < N) {
            *reinterpret_cast<float4*>(gb + (int64_t)n * 3 * AE + AE + 4 * G) = make_float4(dK[u][0], dK[u][1], dK[u][2], dK[u][3]);
            *reinterpret_cast<float4*>(gb + (int64_t)n * 3 * AE + 2 * AE + 4 * G) = make_float4(dV[u][0], dV[u][1], dV[u][2], dV[u][3]);
        }
    }
}

template <int U>
int launch_u(const float* qkv, const float* dout, float* dqkv, int64_t B, int N, hipStream_t st)
{
    const size_t lds = bwd_lds_bytes(N);
    auto k = k_mha_encoder_bwd_mfma<U>;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return EAMRL_E_LAUNCH;
    hipLaunchKernelGGL(k, dim3((unsigned)(B * AH)), dim3(512), lds, st, qkv, dout, dqkv, N);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

}  // namespace

bool mha_encoder_bwd_mfma_supports(int N, int E, int H)
{
    return E == AE && H == AH && N >= 113 && N <= 1024 && bwd_lds_bytes(N) <= 160 * 1024;
}

int launch_mha_encoder_bwd_mfma(const float* qkv, const float* dout, float* dqkv, int64_t B, int N, hipStream_t st)
{
    if (B <= 0) return 0;
    switch (((N + 15) / 16 + 7) / 8) {                  // key tiles per wave
    case 1: return launch_u<1>(qkv, dout, dqkv, B, N, st);
    case 2: return launch_u<2>(qkv, dout, dqkv, B, N, st);
    case 3: return launch_u<3>(qkv, dout, dqkv, B, N, st);
    case 4: return launch_u<4>(qkv, dout, dqkv, B, N, st);
    case 5: return launch_u<5>(qkv, dout, dqkv, B, N, st);
    case 6: return launch_u<6>(qkv, dout, dqkv, B, N, st);
    case 7: return launch_u<7>(qkv, dout, dqkv, B, N, st);
    case 8: return launch_u<8>(qkv, dout, dqkv, B, N, st);
    default: return EAMRL_E_LAUNCH;
    }
}

}  // namespace eamrl
