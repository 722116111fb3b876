// The stages that the three re-evaluation backward kernels share -- k_reeval_bwd_logits and k_reeval_bwd_lp (reeval.hip) and
// k_eas_layer_bwd (eas_layer.hip) -- each stated once, over one 16-query tile.  EAS and PPO reuse the rollout's log-prob as
// the normaliser (derive_lse), so the three kernels must compute z, dz/du and du identically: they call these (one exception,
// with its reason, in k_reeval_bwd_logits).  Every kernel keeps its own LDS map, barriers and pipeline; a stage only names the
// buffers it is handed.
//
// Lane roles: in a score / logit tile lane (query j = lane & 15, group G = lane >> 4) holds keys 16 kt + 4 r + G in register r;
// in a product over the tile's queries lane (column 16 wv + j, G) takes the queries 4 t + G.
#pragma once
#include "mfma_tile.hpp"

namespace eamrl {

constexpr int RE = 128;              // embed dim

__device__ __forceinline__ void load_lp_frags(const ReevalArgs& a, int64_t b, int kt, int lane, float (&lpf)[32])
{
    const int j = lane & 15, G = lane >> 4, n = 16 * kt + 4 * (j & 3) + (j >> 2);
#pragma unroll
    for (int t = 0; t < 32; ++t) lpf[t] = n < a.M ? a.Lp[(b * a.M + n) * a.ld + 4 * t + G] : 0.0f;
}

// u^T tile of key tile kt against the heads tile: A = Lp rows (keys in pi order), B = heads^T
__device__ __forceinline__ f32x4 logit_tile(const float (&lpf)[32], const float* HT, int lane)
{
    const int j = lane & 15, G = lane >> 4;
    const float* hp = HT + j * TS + G * TG;
    f32x4 u = z4();
#pragma unroll
    for (int g4 = 0; g4 < 8; ++g4) {
        const float2 lo = *reinterpret_cast<const float2*>(hp + 4 * g4), hi = *reinterpret_cast<const float2*>(hp + 4 * g4 + 2);
        u = mf(lpf[4 * g4 + 0], lo.x, u);
        u = mf(lpf[4 * g4 + 1], lo.y, u);
        u = mf(lpf[4 * g4 + 2], hi.x, u);
        u = mf(lpf[4 * g4 + 3], hi.y, u);
    }
    return u;
}

// z (processed logit) and dz/du of one accumulator value
__device__ __forceinline__ float process_logit(float u, float clip, float inv_temp, float& dzdu)
{
    u *= 0.08838834764831845f;                      // 1 / sqrt(128)
    float z = u, d = 1.0f;
    if (clip > 0.0f) {
        const float e2 = fexp(2.0f * u);
        const float th = 1.0f - 2.0f / (e2 + 1.0f);
        z = clip * th;
        d = clip * (1.0f - th * th);
    }
    dzdu = d * inv_temp * 0.08838834764831845f;
    return z * inv_temp;
}

// The rollout kept every step's glimpse output (eamrl_state.heads_out): thread (query jq = w's, float4 e4) fetches its share of
// the tile's heads rows.  Branch-free like load_rows (reeval.hip): a query past the chunk's end or before tstart reads a row
// that exists and is masked by `fl` (bit 0: query exists, 3: the step has a heads row) when the tile is staged.
__device__ __forceinline__ void load_heads(const ReevalArgs& a, int64_t b, int s0, int ns, int e4, const QWalk& w, int qi, int& fl,
                                           float4& dh)
{
    const int64_t r = (int64_t)(s0 + min(w.sl, ns - 1)) * a.B + b;
    const int th = max(w.t - a.tstart, 0);
    fl = (qi >= 0 ? 1 : 0) | (w.t >= a.tstart && th < a.heads_T ? 8 : 0);
    dh = *reinterpret_cast<const float4*>(a.heads + (r * a.heads_T + min(th, a.heads_T - 1)) * RE + 4 * e4);
}
__device__ __forceinline__ void stage_heads(int fl, const float4& dh, float* HT, int jq, int e4)
{
    const bool ok = (fl & 9) == 9;
    float* dp = HT + jq * TS + e4;
    dp[0] = ok ? dh.x : 0.0f; dp[TG] = ok ? dh.y : 0.0f; dp[2 * TG] = ok ? dh.z : 0.0f; dp[3 * TG] = ok ? dh.w : 0.0f;
}

// Lp^T fragments of wave wv -> LDS (lpt: this lane's slot, [t4] at stride 64 float4): row e = 16 wv + j, k index = key 4 t + G,
// t = 4 t4 + i -- the A operand of lpt_du
template <int RTT>
__device__ __forceinline__ void fill_lpt(const ReevalArgs& a, int64_t b, int wv, int lane, float4* lpt)
{
    const int j = lane & 15, G = lane >> 4;
#pragma unroll
    for (int t4 = 0; t4 < RTT; ++t4) {
        float kk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = 4 * (4 * t4 + i) + G;
            kk[i] = n < a.M ? a.Lp[(b * a.M + n) * a.ld + 16 * wv + j] : 0.0f;
        }
        lpt[t4 * 64] = make_float4(kk[0], kk[1], kk[2], kk[3]);
    }
}

// Logit-stage backward of one tile.  u: this lane's logit accumulator of key tile wv (own = wv < RTT: the wave has one);
// act / g / lse: the lane's query -- chosen node (-1: no query), glogp (0 unless the step takes a gradient: the caller's `live`
// rule) and the normaliser, or with derive_lse the ROLLOUT's log-prob of the chosen node: the lane that owns that node then
// publishes z[action] - logp through LSE[j], behind a barrier that every thread of the workgroup meets here.
//   du[n] = g (1[n == act] - p[n]) dz/du,  p = exp(z - lse), 0 for an infeasible node  ->  DU[n * DS + j]
// k_reeval_bwd_logits writes the same stage out with its entropy and dynamic-embedding terms (see there).
__device__ __forceinline__ void logit_bwd_tile(const f32x4& u, bool own, int wv, int lane, const uint4& mb, int act, float g, float lse,
                                               bool derive_lse, float clip, float inv_temp, float* LSE, float* DU)
{
    const int j = lane & 15, G = lane >> 4;
    float zr[4] = {0.f, 0.f, 0.f, 0.f}, dz[4] = {0.f, 0.f, 0.f, 0.f};
    if (own) {
#pragma unroll
        for (int r = 0; r < 4; ++r) zr[r] = process_logit(u[r], clip, inv_temp, dz[r]);
    }
    if (derive_lse) {           // the lane that owns the chosen node publishes z[action] - logp for its query
        if (own) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (16 * wv + 4 * r + G == act && g != 0.0f) LSE[j] = zr[r] - lse;
        }
        __syncthreads();
        if (g != 0.0f) lse = LSE[j];
    }
    if (own) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n0 = 16 * wv + 4 * r;
            const uint32_t w = (n0 >> 5) == 0 ? mb.x : (n0 >> 5) == 1 ? mb.y : (n0 >> 5) == 2 ? mb.z : mb.w;
            const bool ok = (w >> ((n0 & 31) + G)) & 1u;
            float du = 0.0f;
            if (ok && g != 0.0f) {
                const float p = fexp(zr[r] - lse);
                du = g * ((n0 + G == act ? 1.0f : 0.0f) - p) * dz[r];
            }
            DU[(n0 + G) * DS + j] = du;
        }
    }
}

// Lp^T . du of the tile: lane (query j, G), register r -> column 16 wv + 4 G + r (dheads in reeval.hip, dY in eas_layer.hip)
template <int RTT>
__device__ __forceinline__ f32x4 lpt_du(const float4* lpt, const float* DU, int lane)
{
    const int j = lane & 15, G = lane >> 4;
    f32x4 d = z4();
#pragma unroll
    for (int t4 = 0; t4 < RTT; ++t4) {
        const float4 ll = lpt[t4 * 64];
        d = mf(ll.x, DU[(16 * t4 + G) * DS + j], d);
        d = mf(ll.y, DU[(16 * t4 + 4 + G) * DS + j], d);
        d = mf(ll.z, DU[(16 * t4 + 8 + G) * DS + j], d);
        d = mf(ll.w, DU[(16 * t4 + 12 + G) * DS + j], d);
    }
    return d;
}

// column c = 16 wv + j of an A-layout tile at this lane's queries 4 t + G: the B operand of a product over the tile's queries
__device__ __forceinline__ void load_tile_col(const float* XT, int wv, int lane, float (&xb)[4])
{
    const int j = lane & 15, G = lane >> 4, c = 16 * wv + j;
#pragma unroll
    for (int t = 0; t < 4; ++t) xb[t] = XT[(4 * t + G) * TS + a_off(c)];
}

// dLp[n][e] += sum_q du[q][n] heads[q][e]: wave wv the embedding columns 16 wv .. 16 wv + 15 of every key tile (hb: load_tile_col of
// the heads tile); lane (column 16 wv + j, G), register r -> key 16 nt + 4 G + r
template <int RTT>
__device__ __forceinline__ void dlp_accumulate(const float* DU, const float (&hb)[4], int lane, f32x4 (&dLp)[RTT])
{
    const int j = lane & 15, G = lane >> 4;
#pragma unroll
    for (int nt = 0; nt < RTT; ++nt)
#pragma unroll
        for (int t = 0; t < 4; ++t) dLp[nt] = mf(DU[(16 * nt + j) * DS + 4 * t + G], hb[t], dLp[nt]);
}
// The caller's buffer is accumulated into and nchunk workgroups share an instance: float atomics
template <int RTT>
__device__ __forceinline__ void dlp_flush(const ReevalArgs& a, int64_t b, int wv, int lane, const f32x4 (&dLp)[RTT])
{
    const int j = lane & 15, G = lane >> 4;
#pragma unroll
    for (int nt = 0; nt < RTT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = 16 * nt + 4 * G + r;
            if (n < a.M) atomicAdd(a.dLp + (b * a.M + n) * a.ldg + 16 * wv + j, dLp[nt][r]);
        }
}

}  // namespace eamrl
