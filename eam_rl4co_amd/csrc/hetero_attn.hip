// Heterogeneous multi-head attention of the HAM encoder (pickup and delivery, Li et al. 2021), forward on fp32 MFMA and backward
// on VALU.
//
// Reference: rl4co/models/zoo/ham/attention.py:53-488 (HeterogenousMHA.forward between the projections and W_out).  Nodes:
// depot 0, pickups 1..P, deliveries P+1..2P, M = 2P + 1; the partner of pickup i is i + P, of delivery i it is i - P.  A row i
// scores every key with its general query q (M scores); a pickup or delivery also scores its partner's key with qpair (1), the
// keys of its own role with qsame (P) and those of the other role with qother (P): 2M scores under ONE softmax, and since all
// groups share k and v,
//   out_i = ( sum_j (w_gen[i][j] + w_x[i][j]) v_j + w_pair[i] v_partner(i) ) / Z_i,
//   w = exp(s - max over all 2M scores),  Z_i = sum_j (w_gen + w_x)[i][j] + w_pair[i],
// where x[i][j] is the ONE extra score a non-depot key j has for a non-depot row i: qsame_i k_j when j has i's role, qother_i k_j
// when it has the other one (-inf, weight exactly 0, for the depot key, the depot row and padded keys).
//
// proj [B][M][6E] = q | k | v | qpair | qsame | qother, each "(h d)"; the depot's last 3E are never read.
//
// Forward: the layout of k_mha_encoder_mfma (encoder_attn_mfma.hip).  One workgroup = (instance, head), 8 wavefronts; the head's
// keys and values are staged once in LDS in MFMA fragment order (KF / VF: stage_kv_fragments of mfma_tile.hpp).  A wavefront takes query tiles of 16 rows.  The
// B operand of a 16x16x4 MFMA is per lane = per query row, so for a key tile that holds keys of one role a lane feeds the query
// its own row has for that role (qsame or qother): one extra score chain per key tile.  The role ranges are not tile-aligned:
// a tile that holds pickups AND deliveries (at most one per head, besides tile 0 of tiny graphs) runs a second chain, and each
// accumulator register picks its key's chain.  Pass 1 takes the row maximum over the general, the extra and the pair score
// before any exp; pass 2 recomputes the scores and feeds w_gen + w_x to the value MFMAs.  The pair term is a 16-wide dot and a
// 16-wide axpy per row on VALU.  No atomics; every sum has a fixed order, so two runs are bit-equal.
#include "mfma_tile.hpp"

namespace eamrl {

namespace {

constexpr int HD = 16;      // head width
constexpr int HE = 128, HH = 8;

__global__ __launch_bounds__(512, 2) void k_hetero_mha(const float* __restrict__ proj, float* __restrict__ out, int M)
{
    constexpr int D = HD, E = HE, H = HH, LD = 6 * HE;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int NT = (M + 15) >> 4;                       // key / query tiles
    const int P = (M - 1) >> 1;
    float* KF = lds;                                    // [NT][64][4]
    float* VF = lds + (size_t)NT * 256;                 // [NT][64][4]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, G = lane >> 4;
    const int64_t b = blockIdx.x / H;
    const int h = (int)(blockIdx.x - b * H);
    const float* base = proj + b * (int64_t)M * LD + h * D;

    stage_kv_fragments(KF, VF, base, LD, E, M, NT);
    __syncthreads();

    for (int qt = wv; qt < NT; qt += 8) {
        // ---- query fragments: lane (row j, G) holds columns 4 t + G, times 1/sqrt(D) = 0.25 --------------------------------------
        const int qrow = 16 * qt + j;
        const int role = (qrow == 0 || qrow >= M) ? 0 : (qrow <= P ? 1 : 2);        // 0: depot (or a padded row)
        const int partner = role == 1 ? qrow + P : (role == 2 ? qrow - P : 0);
        const float* qp = base + (int64_t)(qrow < M ? qrow : M - 1) * LD + G;
        float q[4], qa[4], qb[4], qpair[4];             // qa: against pickup keys, qb: against delivery keys
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            q[t] = qp[4 * t] * 0.25f;
            float same = 0.0f, other = 0.0f;
            qpair[t] = 0.0f;
            if (role) {
                qpair[t] = qp[3 * E + 4 * t] * 0.25f;
                same = qp[4 * E + 4 * t] * 0.25f;
                other = qp[5 * E + 4 * t] * 0.25f;
            }
            qa[t] = role == 1 ? same : other;
            qb[t] = role == 1 ? other : same;
        }
        // ---- pair score: qpair_i . k_partner(i), columns 4 t + G per lane, summed over the four lane groups ----------------------
        float sp = -INFINITY;
        {
            float d = 0.0f;
            if (role) {
                const float* kp = base + (int64_t)partner * LD + E + G;
                d = qpair[0] * kp[0];
                d = fma_(qpair[1], kp[4], d);
                d = fma_(qpair[2], kp[8], d);
                d = fma_(qpair[3], kp[12], d);
            }
            d = lane_groups_sum(d);
            if (role) sp = d;
        }
        // scores of key tiles kt0, kt0 + 1 (clamped), four chains interleaved: sg general, sx extra
        auto scores2 = [&](int kt0, f32x4 (&sg)[2], f32x4 (&sx)[2]) {
            float4 kf[2];
            bool hasP[2], hasD[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int kt = kt0 + u < NT ? kt0 + u : NT - 1;
                kf[u] = *reinterpret_cast<const float4*>(KF + ((size_t)kt * 64 + lane) * 4);
                hasP[u] = 16 * kt <= P;                               // (uniform) the tile holds a pickup key (16 kt + 15 >= 1 always)
                hasD[u] = 16 * kt + 15 > P;                           // (uniform) ... a delivery key (16 kt <= 2 P always)
            }
            float x[2][4];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int t = 0; t < 4; ++t) x[u][t] = hasP[u] ? qa[t] : qb[t];
#pragma unroll
            for (int u = 0; u < 2; ++u) sg[u] = mf(kf[u].x, q[0], (f32x4){0.f, 0.f, 0.f, 0.f});
#pragma unroll
            for (int u = 0; u < 2; ++u) sx[u] = mf(kf[u].x, x[u][0], (f32x4){0.f, 0.f, 0.f, 0.f});
#pragma unroll
            for (int u = 0; u < 2; ++u) sg[u] = mf(kf[u].y, q[1], sg[u]);
#pragma unroll
            for (int u = 0; u < 2; ++u) sx[u] = mf(kf[u].y, x[u][1], sx[u]);
#pragma unroll
            for (int u = 0; u < 2; ++u) sg[u] = mf(kf[u].z, q[2], sg[u]);
#pragma unroll
            for (int u = 0; u < 2; ++u) sx[u] = mf(kf[u].z, x[u][2], sx[u]);
#pragma unroll
            for (int u = 0; u < 2; ++u) sg[u] = mf(kf[u].w, q[3], sg[u]);
#pragma unroll
            for (int u = 0; u < 2; ++u) sx[u] = mf(kf[u].w, x[u][3], sx[u]);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int kt = kt0 + u;
                f32x4 sd = sx[u];                                     // scores against the delivery keys of the tile
                if (hasP[u] && hasD[u]) {                             // (uniform) both roles in one tile: a chain of its own
                    sd = mf(kf[u].x, qb[0], (f32x4){0.f, 0.f, 0.f, 0.f});
                    sd = mf(kf[u].y, qb[1], sd);
                    sd = mf(kf[u].z, qb[2], sd);
                    sd = mf(kf[u].w, qb[3], sd);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = 16 * kt + 4 * r + G;
                    const bool live = kt < NT && key < M;
                    if (!live) sg[u][r] = -INFINITY;
                    sx[u][r] = (live && role && key >= 1) ? (key <= P ? sx[u][r] : sd[r]) : -INFINITY;
                }
            }
        };
        // ---- pass 1: row maxima over the general, extra and pair scores ----------------------------------------------------------
        float m = -INFINITY;
        for (int kt0 = 0; kt0 < NT; kt0 += 2) {
            f32x4 sg[2], sx[2];
            scores2(kt0, sg, sx);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                m = vmax3_raw(m, vmax_raw(sg[u][0], sg[u][1]), vmax_raw(sg[u][2], sg[u][3]));
                m = vmax3_raw(m, vmax_raw(sx[u][0], sx[u][1]), vmax_raw(sx[u][2], sx[u][3]));
            }
        }
        m = vmax_raw(lane_groups_max(m), sp);
        // ---- pass 2: weights, Z partial, value product ---------------------------------------------------------------------------
        f32x4 o = (f32x4){0.f, 0.f, 0.f, 0.f};
        float zp = 0.0f;
        for (int kt0 = 0; kt0 < NT; kt0 += 2) {
            f32x4 sg[2], sx[2];
            scores2(kt0, sg, sx);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (kt0 + u < NT) {                     // (uniform)
                    const float4 vf = *reinterpret_cast<const float4*>(VF + ((size_t)(kt0 + u) * 64 + lane) * 4);
                    const f32x2 g01 = d_expf2_nonpos((f32x2){sg[u][0] - m, sg[u][1] - m});
                    const f32x2 g23 = d_expf2_nonpos((f32x2){sg[u][2] - m, sg[u][3] - m});
                    const f32x2 x01 = d_expf2_nonpos((f32x2){sx[u][0] - m, sx[u][1] - m});
                    const f32x2 x23 = d_expf2_nonpos((f32x2){sx[u][2] - m, sx[u][3] - m});
                    const float w0 = g01.x + x01.x, w1 = g01.y + x01.y, w2 = g23.x + x23.x, w3 = g23.y + x23.y;
                    zp = zp + w0; zp = zp + w1; zp = zp + w2; zp = zp + w3;
                    o = mf(vf.x, w0, o);
                    o = mf(vf.y, w1, o);
                    o = mf(vf.z, w2, o);
                    o = mf(vf.w, w3, o);
                }
            }
        }
        zp = lane_groups_sum(zp);
        // ---- pair term; o: lane (row j, G), register r -> head column 4 G + r -----------------------------------------------------
        if (qrow < M) {
            if (role) {
                const float wp = d_expf(sp - m);
                const float4 vp = *reinterpret_cast<const float4*>(base + (int64_t)partner * LD + 2 * E + 4 * G);
                zp = zp + wp;
                o[0] = fma_(wp, vp.x, o[0]); o[1] = fma_(wp, vp.y, o[1]); o[2] = fma_(wp, vp.z, o[2]); o[3] = fma_(wp, vp.w, o[3]);
            }
            *reinterpret_cast<float4*>(out + (b * M + qrow) * (int64_t)E + h * D + 4 * G) =
                make_float4(o[0] / zp, o[1] / zp, o[2] / zp, o[3] / zp);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Backward (VALU).  One workgroup = (instance, head); q (scaled), k, v, the three extra queries (scaled) and dout of the head in
// LDS.  The softmax is recomputed from proj, nothing else is kept (as k_mha_encoder_bwd).  With p = the softmax weights,
// dp[i][j] = dout_i . v_j and delta_i = dout_i . out_i = sum over all 2M weights of p dp:
//   ds = p (dp - delta);  dq_i = c sum_j ds_gen k_j;  dqsame_i / dqother_i = c sum over the keys of the same / other role of ds_x k_j;
//   dqpair_i = c ds_pair k_partner(i);  dv_j = sum_i (p_gen + p_x)[i][j] dout_i + p_pair[partner(j)] dout_partner(j);
//   dk_j = c ( sum_i ds_gen[i][j] q_i + ds_x[i][j] (qsame_i or qother_i) + ds_pair[partner(j)] qpair_partner(j) ).
// Row side: a thread owns a row i (max, Z and out, then the four query gradients).  Key side: a thread owns a key j and walks the
// rows in ascending order (dk, dv): fixed summation order, no atomics.  Every weight is recomputed by the same function from the
// same operands on both sides, so both see the same bits.
// ------------------------------------------------------------------------------------------------------------------------------------
constexpr int BS = 17;      // LDS row stride (16 + 1: a thread per row walks its row without bank conflicts)

__device__ __forceinline__ float dot16(const float* a, const float* b)
{
    float d = a[0] * b[0];
#pragma unroll
    for (int c = 1; c < 16; ++c) d = fma_(a[c], b[c], d);
    return d;
}

// dot16 of (first ? a : b) with k: element-wise selects, so both register arrays stay in registers
__device__ __forceinline__ float dot16_sel(bool first, const float (&a)[16], const float (&b)[16], const float* k)
{
    float d = (first ? a[0] : b[0]) * k[0];
#pragma unroll
    for (int c = 1; c < 16; ++c) d = fma_(first ? a[c] : b[c], k[c], d);
    return d;
}

__device__ __forceinline__ int node_role(int i, int P) { return i == 0 ? 0 : (i <= P ? 1 : 2); }

__global__ __launch_bounds__(192) void k_hetero_mha_bwd(const float* __restrict__ proj, const float* __restrict__ dout,
                                                         float* __restrict__ dproj, int M)
{
    constexpr int D = HD, E = HE, H = HH, LD = 6 * HE;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int P = (M - 1) >> 1;
    float* Q = lds;                     // [M][BS] each
    float* K = Q + (size_t)M * BS;
    float* V = K + (size_t)M * BS;
    float* Qp = V + (size_t)M * BS;
    float* Qs = Qp + (size_t)M * BS;
    float* Qo = Qs + (size_t)M * BS;
    float* dO = Qo + (size_t)M * BS;
    float* rmax = dO + (size_t)M * BS;  // [M] each: row maximum, 1 / Z, delta, ds_pair, p_pair
    float* rinv = rmax + M;
    float* rdel = rinv + M;
    float* rdsp = rdel + M;
    float* rpp = rdsp + M;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / H;
    const int h = (int)(blockIdx.x - b * H);
    const float* base = proj + b * (int64_t)M * LD + h * D;
    float* gbase = dproj + b * (int64_t)M * LD + h * D;
    const float* dbase = dout + b * (int64_t)M * E + h * D;

    for (int x = tid; x < M * D; x += blockDim.x) {
        const int n = x >> 4, c = x & 15;
        const float* p = base + (int64_t)n * LD + c;
        Q[n * BS + c] = p[0] * 0.25f;
        K[n * BS + c] = p[E];
        V[n * BS + c] = p[2 * E];
        const bool nd = n != 0;
        Qp[n * BS + c] = nd ? p[3 * E] * 0.25f : 0.0f;
        Qs[n * BS + c] = nd ? p[4 * E] * 0.25f : 0.0f;
        Qo[n * BS + c] = nd ? p[5 * E] * 0.25f : 0.0f;
        dO[n * BS + c] = dbase[(int64_t)n * E + c];
    }
    __syncthreads();

    // ---- row side -------------------------------------------------------------------------------------------------------------------
    for (int i = tid; i < M; i += blockDim.x) {
        const int ri = node_role(i, P);
        const int pi = ri == 1 ? i + P : (ri == 2 ? i - P : 0);
        float q[16], qs[16], qo[16], g[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) { q[c] = Q[i * BS + c]; qs[c] = Qs[i * BS + c]; qo[c] = Qo[i * BS + c]; g[c] = dO[i * BS + c]; }
        const float sp = ri ? dot16(Qp + i * BS, K + pi * BS) : -INFINITY;
        float m = sp;
        for (int jj = 0; jj < M; ++jj) {
            m = fmaxf(m, dot16(q, K + jj * BS));
            if (ri && jj) m = fmaxf(m, dot16_sel(node_role(jj, P) == ri, qs, qo, K + jj * BS));
        }
        float z = 0.0f, o[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) o[c] = 0.0f;
        for (int jj = 0; jj < M; ++jj) {
            float w = d_expf(dot16(q, K + jj * BS) - m);
            if (ri && jj) w = w + d_expf(dot16_sel(node_role(jj, P) == ri, qs, qo, K + jj * BS) - m);
            z = z + w;
#pragma unroll
            for (int c = 0; c < 16; ++c) o[c] = fma_(w, V[jj * BS + c], o[c]);
        }
        const float wp = ri ? d_expf(sp - m) : 0.0f;
        z = z + wp;
        const float inv = 1.0f / z;
        float delta = 0.0f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            o[c] = fma_(wp, V[pi * BS + c], o[c]) * inv;
            delta = fma_(g[c], o[c], delta);
        }
        const float ppair = wp * inv;
        const float dsp = ri ? ppair * (dot16(g, V + pi * BS) - delta) : 0.0f;
        rmax[i] = m; rinv[i] = inv; rdel[i] = delta; rdsp[i] = dsp; rpp[i] = ppair;
        // query gradients
        float dq[16], dqs[16], dqo[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) dq[c] = dqs[c] = dqo[c] = 0.0f;
        for (int jj = 0; jj < M; ++jj) {
            const float dp = dot16(g, V + jj * BS) - delta;
            const float dsg = d_expf(dot16(q, K + jj * BS) - m) * inv * dp;
#pragma unroll
            for (int c = 0; c < 16; ++c) dq[c] = fma_(dsg, K[jj * BS + c], dq[c]);
            if (ri && jj) {
                const bool same = node_role(jj, P) == ri;
                const float dsx = d_expf(dot16_sel(same, qs, qo, K + jj * BS) - m) * inv * dp;
                if (same) {
#pragma unroll
                    for (int c = 0; c < 16; ++c) dqs[c] = fma_(dsx, K[jj * BS + c], dqs[c]);
                } else {
#pragma unroll
                    for (int c = 0; c < 16; ++c) dqo[c] = fma_(dsx, K[jj * BS + c], dqo[c]);
                }
            }
        }
        float* gp = gbase + (int64_t)i * LD;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            gp[c] = dq[c] * 0.25f;
            gp[3 * E + c] = ri ? dsp * K[pi * BS + c] * 0.25f : 0.0f;      // the depot's three extra gradients are zeros
            gp[4 * E + c] = dqs[c] * 0.25f;
            gp[5 * E + c] = dqo[c] * 0.25f;
        }
    }
    __syncthreads();

    // ---- key side: rows in ascending order -----------------------------------------------------------------------------------------
    for (int jj = tid; jj < M; jj += blockDim.x) {
        const int rj = node_role(jj, P);
        const int pj = rj == 1 ? jj + P : (rj == 2 ? jj - P : 0);
        float k[16], v[16], dk[16], dv[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) { k[c] = K[jj * BS + c]; v[c] = V[jj * BS + c]; dk[c] = dv[c] = 0.0f; }
        for (int i = 0; i < M; ++i) {
            const int ri = node_role(i, P);
            const float m = rmax[i], inv = rinv[i];
            const float dp = dot16(dO + i * BS, v) - rdel[i];
            const float pg = d_expf(dot16(Q + i * BS, k) - m) * inv;
            float pw = pg;
            const float dsg = pg * dp;
#pragma unroll
            for (int c = 0; c < 16; ++c) dk[c] = fma_(dsg, Q[i * BS + c], dk[c]);
            if (ri && rj) {
                const float* qx = (ri == rj ? Qs : Qo) + i * BS;
                const float px = d_expf(dot16(qx, k) - m) * inv;
                const float dsx = px * dp;
                pw = pw + px;
#pragma unroll
                for (int c = 0; c < 16; ++c) dk[c] = fma_(dsx, qx[c], dk[c]);
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) dv[c] = fma_(pw, dO[i * BS + c], dv[c]);
        }
        if (rj) {                       // the pair term of the partner row
            const float dsp = rdsp[pj], pp = rpp[pj];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                dk[c] = fma_(dsp, Qp[pj * BS + c], dk[c]);
                dv[c] = fma_(pp, dO[pj * BS + c], dv[c]);
            }
        }
        float* gp = gbase + (int64_t)jj * LD;
#pragma unroll
        for (int c = 0; c < 16; ++c) { gp[E + c] = dk[c]; gp[2 * E + c] = dv[c]; }
    }
}

}  // namespace

bool hetero_mha_supports(int M, int E, int H)
{
    return E == HE && H == HH && M >= 3 && (M & 1) && M <= EAMRL_HETERO_MHA_MAX_NODES;
}

bool hetero_mha_bwd_supports(int M, int E, int H)
{
    return E == HE && H == HH && M >= 3 && (M & 1) && M <= EAMRL_HETERO_MHA_BWD_MAX_NODES;
}

int launch_hetero_mha(const float* proj, float* out, int64_t B, int M, hipStream_t st)
{
    const int NT = (M + 15) >> 4;
    const size_t lds = (size_t)NT * 512 * sizeof(float);
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(k_hetero_mha),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return EAMRL_E_LAUNCH;
    hipLaunchKernelGGL(k_hetero_mha, dim3((unsigned)(B * HH)), dim3(512), lds, st, proj, out, M);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

int launch_hetero_mha_bwd(const float* proj, const float* dout, float* dproj, int64_t B, int M, hipStream_t st)
{
    const size_t lds = ((size_t)M * BS * 7 + (size_t)M * 5) * sizeof(float);
    if (lds > 64 * 1024) return EAMRL_E_ARG;
    hipLaunchKernelGGL(k_hetero_mha_bwd, dim3((unsigned)(B * HH)), dim3(192), lds, st, proj, dout, dproj, M);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

}  // namespace eamrl
