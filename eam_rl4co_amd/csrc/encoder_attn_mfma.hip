// Encoder self-attention for graphs too large for the fused kernel (N > 112, e.g. CVRP-500: N = 501) on fp32 MFMA, keys
// tiled through LDS (round 3; VERDICT r2 item 8: the VALU kernel k_mha_encoder_tiled took 2.3 ms per layer at 512 x 501).
//
// Reference: rl4co/models/nn/attention.py:66-136 (MultiHeadAttention.forward: scaled_dot_product_attention over the packed
// projection "b s (three h d)").  Arithmetic = the canonical order of DESIGN.md 2, bit for bit k_mha_encoder_tiled / the
// oracle's orc_mha_encoder:
//   s = chain_d(q * 0.25, k) (the power-of-two scale folded into q), w = d_expf(s - max over all keys),
//   Z = (P0 + P1) + (P2 + P3), P_r = sequential sum of w over the keys j = r (mod 4) ascending, o = chain_j(w, v) / Z.
//
// One workgroup = (instance, head), 8 wavefronts.  The head's keys and values (N x 16 floats each) are staged ONCE in LDS in
// MFMA fragment order (KF / VF: stage_kv_fragments of mfma_tile.hpp states the layout).
// A wavefront takes query tiles qt = wave, wave + 8, ...: pass 1 walks the key tiles for the row maxima (4 MFMAs per tile, four
// tiles' chains interleaved: the f32 16x16x4 MFMA has a 40-cycle dependent latency against a 32-cycle issue interval), pass 2
// walks them again in ascending order for exp / Z / PV, so every sum keeps the canonical ascending-key order (the accumulators
// simply carry across tiles).  Keys >= N get -inf scores (weight exactly 0) and zero values.
#include "mfma_tile.hpp"

namespace eamrl {

namespace {

__global__ __launch_bounds__(512, 2) void k_mha_encoder_mfma(const float* __restrict__ qkv, float* __restrict__ out, int N, int E, int H)
{
    constexpr int D = 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int NT = (N + 15) >> 4;                       // key / query tiles
    float* KF = lds;                                    // [NT][64][4]
    float* VF = lds + (size_t)NT * 256;                 // [NT][64][4]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, G = lane >> 4;
    const int64_t b = blockIdx.x / H;
    const int h = (int)(blockIdx.x - b * H);
    const float* base = qkv + b * (int64_t)N * 3 * E + h * D;

    stage_kv_fragments(KF, VF, base, 3 * E, E, N, NT);
    __syncthreads();

    for (int qt = wv; qt < NT; qt += 8) {
        // ---- query fragment: lane (query j, G): q[16 qt + j][4 t + G] * 0.25 ----------------------------------------------------
        const int qrow = 16 * qt + j;
        const float* qp = base + (int64_t)(qrow < N ? qrow : N - 1) * 3 * E + G;
        const float q0 = qp[0] * 0.25f, q1 = qp[4] * 0.25f, q2 = qp[8] * 0.25f, q3 = qp[12] * 0.25f;
        auto scores4 = [&](int kt0, f32x4 (&s)[4]) {    // tiles kt0 .. kt0 + 3 (clamped), chains interleaved
            float4 kf[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kt = kt0 + u < NT ? kt0 + u : NT - 1;
                kf[u] = *reinterpret_cast<const float4*>(KF + ((size_t)kt * 64 + lane) * 4);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] = mf(kf[u].x, q0, (f32x4){0.f, 0.f, 0.f, 0.f});
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] = mf(kf[u].y, q1, s[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] = mf(kf[u].z, q2, s[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] = mf(kf[u].w, q3, s[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kt = kt0 + u;
                if (16 * kt + 16 > N) {                 // (uniform) the tile holds padded keys, or lies beyond the last tile
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kt >= NT || 16 * kt + 4 * r + G >= N) s[u][r] = -INFINITY;
                }
            }
        };
        // ---- pass 1: row maxima ------------------------------------------------------------------------------------------------
        float m = -INFINITY;
        for (int kt0 = 0; kt0 < NT; kt0 += 4) {
            f32x4 s[4];
            scores4(kt0, s);
#pragma unroll
            for (int u = 0; u < 4; ++u) m = vmax3_raw(m, vmax_raw(s[u][0], s[u][1]), vmax_raw(s[u][2], s[u][3]));
        }
        m = lane_groups_max(m);                         // the four lane groups G share a query: lanes l, l^16, l^32, l^48
        // ---- pass 2: weights, Z partial (this lane's keys are one residue class mod 4, ascending), value product ------------------
        f32x4 o = (f32x4){0.f, 0.f, 0.f, 0.f};
        float zp = 0.0f;
        for (int kt0 = 0; kt0 < NT; kt0 += 4) {
            f32x4 s[4];
            scores4(kt0, s);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (kt0 + u < NT) {                     // (uniform)
                    const float4 vf = *reinterpret_cast<const float4*>(VF + ((size_t)(kt0 + u) * 64 + lane) * 4);
                    const f32x2 e01 = d_expf2_nonpos((f32x2){s[u][0] - m, s[u][1] - m});
                    const f32x2 e23 = d_expf2_nonpos((f32x2){s[u][2] - m, s[u][3] - m});
                    zp = zp + e01.x; zp = zp + e01.y; zp = zp + e23.x; zp = zp + e23.y;
                    o = mf(vf.x, e01.x, o);
                    o = mf(vf.y, e01.y, o);
                    o = mf(vf.z, e23.x, o);
                    o = mf(vf.w, e23.y, o);
                }
            }
        }
        zp = lane_groups_sum(zp);                       // (P0 + P1) + (P2 + P3) over the lane groups
        // o: lane (query j, G), register r -> head column 4 G + r
        if (qrow < N)
            *reinterpret_cast<float4*>(out + (b * N + qrow) * (int64_t)E + h * D + 4 * G) =
                make_float4(o[0] / zp, o[1] / zp, o[2] / zp, o[3] / zp);
    }
}

}  // namespace

bool mha_encoder_mfma_supports(int N, int E, int H)
{
    const int NT = (N + 15) >> 4;
    return E == 128 && H == 8 && N >= 1 && (size_t)NT * 512 * sizeof(float) <= 150 * 1024;
}

int launch_mha_encoder_mfma(const float* qkv, float* out, int64_t B, int N, int E, int H, hipStream_t st)
{
    const int NT = (N + 15) >> 4;
    const size_t lds = (size_t)NT * 512 * sizeof(float);
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(k_mha_encoder_mfma),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return EAMRL_E_LAUNCH;
    hipLaunchKernelGGL(k_mha_encoder_mfma, dim3((unsigned)(B * H)), dim3(512), lds, st, qkv, out, N, E, H);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

}  // namespace eamrl
