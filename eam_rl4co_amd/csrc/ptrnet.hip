// Pointer Network (Vinyals 2015 / Bello 2016; rl4co/models/zoo/ptrnet) for TSP, E = H = 128, 2 <= N <= 128.
//
//   k_ptrnet_fold      weight-only constants: the rank-2 input part of an LSTM, W_ih (x emb_0 + y emb_1) = x U0 + y U1, as the two
//                      512-vectors U0 = W_ih emb_0, U1 = W_ih emb_1, the bias sum b_ih + b_hh, and (decoder) W_ih decoder_in_0 + b
//   k_ptrnet_encode    the encoder recurrence, all N steps in one launch; 16 instances per workgroup, h W_hh^T as a
//                      [16 x 128] x [128 x 512] product on v_mfma_f32_16x16x4_f32
//   k_ptrnet_rollout   the decode loop, all N steps in one launch; 4 instances per workgroup
//
// Both recurrent kernels run 4 wavefronts; wavefront w owns the hidden units 32 w .. 32 w + 31, i.e. the 8 gate-column tiles
// (gate q = i f g o, half u) -> columns 128 q + 32 w + 16 u + (lane & 15), so that the four gates of one (instance, unit) land in
// the same accumulator slot of the same lane and the cell state never leaves its registers.  W_hh (256 KiB, more than the LDS)
// stays in the register file for the whole launch as the MFMA B operand: 8 tiles x 32 k-steps = 256 registers per lane, which is
// why a workgroup is exactly one wavefront per SIMD (512 registers each).  h is kept in LDS k-major ([k][16 rows]), which is the A
// operand's order: lane l reads element 64 ks + l of it at k-step ks.
//
// The decode step is dominated by the two additive attentions, 2 N 128 tanh per instance (about 40 VALU operations each through
// d_tanhf4), not by the products: 4 instances per workgroup (MFMA rows 4..15 are zero padding) put a batch of 1024 on 256
// compute units, and wavefront w then IS instance w for the attentions: lane l scores the nodes l and l + 64 against the refs,
// which are re-read from L2 / HBM every step (an instance's two ref sets are 128 KiB at N = 128; four would not fit the LDS),
// double-buffered in 16-float chunks.  The LDS holds the two query-projection weights instead, in MFMA fragment order.
//
// Arithmetic: sigmoid = 1 / (1 + d_expf(-x)), tanh / exp / log the defined functions of dmath.hpp; -ffp-contract=off.
#include "mfma_tile.hpp"

namespace eamrl {

namespace {

constexpr int PH = 128;              // hidden = embedding width
constexpr int PG = 4 * PH;           // gate columns
constexpr int ENC_TILE = 16;         // instances per workgroup, encoder
constexpr int DEC_TILE = 4;          // instances per workgroup, rollout
constexpr int NMAX = 128;
constexpr int WS_ENC = 0, WS_DEC = 3 * PG;      // workspace: enc U0 U1 b | dec U0 U1 b V0b
constexpr size_t ROLLOUT_LDS = sizeof(float) * (2 * PH * PH + 2 * PH * 16 + DEC_TILE * PH + 2 * PH + DEC_TILE * NMAX
                                                + DEC_TILE * NMAX * 2 + DEC_TILE * 2);

__device__ __forceinline__ float d_sigmoidf(float x) { return 1.0f / (1.0f + d_expf(0.0f - x)); }

__global__ __launch_bounds__(256) void k_ptrnet_fold(const float* __restrict__ w_ih, const float* __restrict__ b_ih,
                                                     const float* __restrict__ b_hh, const float* __restrict__ emb,
                                                     const float* __restrict__ in0, float* __restrict__ out)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= PG) return;
    const float* wr = w_ih + (size_t)c * PH;
    float u0 = 0.0f, u1 = 0.0f, v0 = 0.0f;
    for (int k = 0; k < PH; ++k) {
        u0 = fma_(wr[k], emb[k], u0);
        u1 = fma_(wr[k], emb[PH + k], u1);
        if (in0) v0 = fma_(wr[k], in0[k], v0);
    }
    const float b = b_ih[c] + b_hh[c];
    out[c] = u0;
    out[PG + c] = u1;
    out[2 * PG + c] = b;
    if (in0) out[3 * PG + c] = v0 + b;
}

// this lane's share of W_hh as MFMA B fragments: tile tt = 2 q + u, k-step ks -> W_hh[column(tt)][4 ks + (lane >> 4)]
__device__ __forceinline__ int gate_col(int tt, int wv, int cl) { return (tt >> 1) * PH + 32 * wv + 16 * (tt & 1) + cl; }

__device__ __forceinline__ void load_whh(float (&w)[8][32], const float* __restrict__ w_hh, int wv, int cl, int kg)
{
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) {
        const float* wr = w_hh + (size_t)gate_col(tt, wv, cl) * PH + kg;
#pragma unroll
        for (int ks = 0; ks < 32; ++ks) w[tt][ks] = wr[4 * ks];
    }
}

// acc[tt] += hT (A, k-major in LDS) x the register-held W_hh fragments
__device__ __forceinline__ void lstm_gemm(const float (&w)[8][32], const float* hT, int lane, f32x4 (&acc)[8])
{
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
        const float av = hT[64 * ks + lane];
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) acc[tt] = mf(av, w[tt][ks], acc[tt]);
    }
}

// the cell: gates i f g o of one (instance, unit) -> new c (in place) and h
__device__ __forceinline__ float lstm_cell(float gi, float gf, float gg, float go, float& c)
{
    const float i_ = d_sigmoidf(gi), f_ = d_sigmoidf(gf), g_ = d_tanhf(gg), o_ = d_sigmoidf(go);
    c = f_ * c + i_ * g_;
    return o_ * d_tanhf(c);
}

__global__ __launch_bounds__(256) void k_ptrnet_encode(eamrl_ptrnet a)
{
    __shared__ float hT[2][PH * 16];
    __shared__ float xy[ENC_TILE * NMAX * 2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, cl = lane & 15, kg = lane >> 4;
    const int N = a.N;
    const int64_t B = a.B, b0 = (int64_t)blockIdx.x * ENC_TILE;
    const float* fold = a.ws + WS_ENC;

    float w[8][32];
    load_whh(w, a.enc_w_hh, wv, cl, kg);
    float u0[8], u1[8], bb[8];
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) {
        const int col = gate_col(tt, wv, cl);
        u0[tt] = fold[col]; u1[tt] = fold[PG + col]; bb[tt] = fold[2 * PG + col];
    }
    for (int i = tid; i < ENC_TILE * 2 * N; i += 256) {
        const int inst = i / (2 * N), r = i - inst * 2 * N;
        const int64_t b = (b0 + inst < B) ? b0 + inst : B - 1;
        xy[inst * (2 * NMAX) + r] = a.locs[b * 2 * N + r];
    }
    for (int i = tid; i < 2 * PH * 16; i += 256) (&hT[0][0])[i] = 0.0f;
    float c[2][4], hl[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) { c[u][i] = 0.0f; hl[u][i] = 0.0f; }
    __syncthreads();

    for (int n = 0; n < N; ++n) {
        const float* hc = hT[n & 1];
        float* hn = hT[(n + 1) & 1];
        f32x4 acc[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float lx = xy[(4 * kg + i) * (2 * NMAX) + 2 * n], ly = xy[(4 * kg + i) * (2 * NMAX) + 2 * n + 1];
#pragma unroll
            for (int tt = 0; tt < 8; ++tt) acc[tt][i] = fma_(ly, u1[tt], fma_(lx, u0[tt], bb[tt]));
        }
        lstm_gemm(w, hc, lane, acc);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int unit = 32 * wv + 16 * u + cl;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int inst = 4 * kg + i;
                const float h = lstm_cell(acc[u][i], acc[2 + u][i], acc[4 + u][i], acc[6 + u][i], c[u][i]);
                hl[u][i] = h;
                hn[unit * 16 + inst] = h;
                if (b0 + inst < B) a.ctx[((b0 + inst) * N + n) * PH + unit] = h;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int unit = 32 * wv + 16 * u + cl;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int inst = 4 * kg + i;
            if (b0 + inst < B) {
                a.h[(b0 + inst) * PH + unit] = hl[u][i];
                a.c[(b0 + inst) * PH + unit] = c[u][i];
            }
        }
    }
}

// q = W x + b for the workgroup's rows: A = xT (k-major LDS tile), B = this wavefront's two column tiles of W, staged once per
// launch in LDS in fragment order (wf: element (tile * 32 + ks) * 64 + lane = W[16 tile + (lane & 15)][4 ks + (lane >> 4)]);
// rows 0 .. DEC_TILE - 1 (lane group 0) go to q [DEC_TILE][PH]
__device__ __forceinline__ void query_proj(const float* wf, const float* __restrict__ bias, const float* xT, float* q, int lane,
                                           int wv, int cl, int kg)
{
    f32x4 acc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const float bv = bias[32 * wv + 16 * u + cl];
        acc[u] = (f32x4){bv, bv, bv, bv};
    }
    const float* w0 = wf + (2 * wv) * 32 * 64 + lane;
    const float* w1 = w0 + 32 * 64;
#pragma unroll 8
    for (int ks = 0; ks < 32; ++ks) {
        const float av = xT[64 * ks + lane];
        acc[0] = mf(av, w0[64 * ks], acc[0]);
        acc[1] = mf(av, w1[64 * ks], acc[1]);
    }
    if (kg == 0) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int i = 0; i < DEC_TILE; ++i) q[i * PH + 32 * wv + 16 * u + cl] = acc[u][i];
    }
}

// stage W [128][128] (row-major, [out][in]) as the fragments query_proj reads
__device__ __forceinline__ void stage_query_weight(const float* __restrict__ W, float* wf, int tid)
{
    for (int i = tid; i < PH * PH; i += 256) {
        const int tile = i >> 11, ks = (i >> 6) & 31, l = i & 63;
        wf[i] = W[(16 * tile + (l & 15)) * PH + 4 * ks + (l >> 4)];
    }
}

// v . tanh(q + e_n) for one node's row e; four interleaved partial sums over d.
// The rows come from L2 / HBM and a workgroup is one wavefront per SIMD, so nothing else hides the load latency: 16-float chunks
// are double-buffered, chunk c + 1 in flight under the tanh of chunk c.
__device__ __forceinline__ void attn_chunk(const f32x4 (&b)[4], const float* q, const float* v, int d0, f32x4& p)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 qq = *reinterpret_cast<const f32x4*>(q + d0 + 4 * j), vv = *reinterpret_cast<const f32x4*>(v + d0 + 4 * j);
        p = pk_fma4(vv, d_tanhf4(qq + b[j]), p);
    }
}
__device__ __forceinline__ void load_chunk(f32x4 (&b)[4], const float* __restrict__ e, int d0)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const f32x4*>(e + d0 + 4 * j);
}
__device__ __forceinline__ float attn_score(const float* __restrict__ e, const float* q, const float* v)
{
    f32x4 p = z4();
    f32x4 a[4], b[4];
    load_chunk(a, e, 0);
#pragma unroll 1
    for (int d = 0; d < PH; d += 32) {
        load_chunk(b, e, d + 16);
        attn_chunk(a, q, v, d, p);
        if (d + 32 < PH) load_chunk(a, e, d + 32);
        attn_chunk(b, q, v, d + 16, p);
    }
    return (p[0] + p[1]) + (p[2] + p[3]);
}

__global__ __launch_bounds__(256) void k_ptrnet_rollout(eamrl_ptrnet a, int mode, const float* __restrict__ noise,
                                                        const int64_t* __restrict__ given, int use_rng, uint64_t seed,
                                                        int64_t* __restrict__ actions, float* __restrict__ logp)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* wq = lds;                                 // [2][PH * PH] query weights of the glimpse / the pointer, fragment order
    float* hT = wq + 2 * PH * PH;                    // [PH][16]
    float* gT = hT + PH * 16;                        // [PH][16]
    float* q = gT + PH * 16;                         // [DEC_TILE][PH]
    float* vv = q + DEC_TILE * PH;                   // [2][PH]
    float* pb = vv + 2 * PH;                         // [DEC_TILE][NMAX]
    float* xy = pb + DEC_TILE * NMAX;                // [DEC_TILE][NMAX][2]
    float* selxy = xy + DEC_TILE * NMAX * 2;         // [DEC_TILE][2]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, cl = lane & 15, kg = lane >> 4;
    const int N = a.N;
    const int64_t B = a.B, b0 = (int64_t)blockIdx.x * DEC_TILE;
    const float* fold = a.ws + WS_DEC;

    float w[8][32];
    load_whh(w, a.dec_w_hh, wv, cl, kg);
    for (int i = tid; i < DEC_TILE * 2 * N; i += 256) {
        const int inst = i / (2 * N), r = i - inst * 2 * N;
        const int64_t b = (b0 + inst < B) ? b0 + inst : B - 1;
        xy[inst * (2 * NMAX) + r] = a.locs[b * 2 * N + r];
    }
    for (int i = tid; i < PH * 16; i += 256) {
        const int k = i >> 4, inst = i & 15;
        const int64_t b = (b0 + inst < B) ? b0 + inst : B - 1;
        hT[i] = inst < DEC_TILE ? a.h[b * PH + k] : 0.0f;
        gT[i] = 0.0f;
    }
    if (tid < PH) { vv[tid] = a.g_v[tid]; vv[PH + tid] = a.p_v[tid]; }
    if (tid < DEC_TILE * 2) selxy[tid] = 0.0f;
    stage_query_weight(a.g_wq, wq, tid);
    stage_query_weight(a.p_wq, wq + PH * PH, tid);
    float c[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t b = (b0 + i < B) ? b0 + i : B - 1;
            c[u][i] = a.c[b * PH + 32 * wv + 16 * u + cl];
        }
    // attention role: wavefront wv is instance b0 + wv, this lane scores the nodes n0 = lane and n1 = lane + 64
    const bool bvalid = b0 + wv < B;
    const int64_t bi = bvalid ? b0 + wv : B - 1;
    const int n0 = lane, n1 = lane + 64;
    const bool in0 = n0 < N, in1 = n1 < N;
    const bool two = N > 64;                                        // uniform: the second node round exists
    const size_t r0 = ((size_t)bi * N + (in0 ? n0 : N - 1)) * PH, r1 = ((size_t)bi * N + (in1 ? n1 : N - 1)) * PH;
    bool vis0 = !in0, vis1 = !in1;                                  // nodes beyond N count as visited
    __syncthreads();

    for (int t = 0; t < N; ++t) {
        // ---- LSTM cell on the tile ---------------------------------------------------------------------------------------------
        // the input part (fold: x U0 + y U1 + b of the node just chosen, W_ih decoder_in_0 + b at step 0) is added after the
        // product; its 24 values per lane are fetched per step (L1 / L2 hits, in flight under the MFMAs) instead of living in
        // registers through the attentions.  The empty asm keeps the compiler from hoisting the loads out of the step loop.
        int fo = (t == 0) ? 3 * PG : 0;
        asm volatile("" : "+v"(fo));
        float fa[8], fb[8], fc[8];
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) {
            const float* f = fold + fo + gate_col(tt, wv, cl);
            fa[tt] = f[0];
            fb[tt] = (t == 0) ? 0.0f : f[PG];
            fc[tt] = (t == 0) ? 0.0f : f[2 * PG];
        }
        f32x4 acc[8];
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) acc[tt] = z4();
        lstm_gemm(w, hT, lane, acc);
        __syncthreads();                                            // every wavefront has read hT
        if (kg == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float lx = selxy[2 * i], ly = selxy[2 * i + 1];
                float gin[8];
#pragma unroll
                for (int tt = 0; tt < 8; ++tt)
                    gin[tt] = acc[tt][i] + ((t == 0) ? fa[tt] : fma_(ly, fb[tt], fma_(lx, fa[tt], fc[tt])));
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    hT[(32 * wv + 16 * u + cl) * 16 + i] = lstm_cell(gin[u], gin[2 + u], gin[4 + u], gin[6 + u], c[u][i]);
            }
        }
        __syncthreads();
        // ---- glimpse: query, scores, masked softmax, readout over the projected refs ----------------------------------------------
        query_proj(wq, a.g_bq, hT, q, lane, wv, cl, kg);
        __syncthreads();
        {
            float s0 = attn_score(a.e_g + r0, q + wv * PH, vv), s1 = 0.0f;
            if (two) s1 = attn_score(a.e_g + r1, q + wv * PH, vv);
            s0 = vis0 ? -INFINITY : s0;
            s1 = vis1 ? -INFINITY : s1;
            const float mx = wave_max(vmax_raw(s0, s1));
            const float x0 = vis0 ? 0.0f : d_expf(s0 - mx), x1 = vis1 ? 0.0f : d_expf(s1 - mx);
            const float Z = wave_tree_sum(x0 + x1);
            pb[wv * NMAX + n0] = x0 / Z;
            pb[wv * NMAX + n1] = x1 / Z;
        }
        __syncthreads();
        {
            // readout: lane = (node parity, 4 columns); the two parities meet through the 32-lane swap
            const float* eg = a.e_g + (size_t)bi * N * PH + 4 * (lane & 31);
            const float* pw = pb + wv * NMAX;
            f32x4 g = z4();
#pragma unroll 4
            for (int n = lane >> 5; n < N; n += 2) g = pk_fma4(splat4(pw[n]), *reinterpret_cast<const f32x4*>(eg + (size_t)n * PH), g);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float tot = g[j] + __shfl_xor(g[j], 32, 64);
                if (lane < 32) gT[(4 * lane + j) * 16 + wv] = tot;
            }
        }
        __syncthreads();
        // ---- pointer: query from the glimpse, clipped scores, log-softmax, selection -----------------------------------------------
        query_proj(wq + PH * PH, a.p_bq, gT, q, lane, wv, cl, kg);
        __syncthreads();
        {
            float s0 = attn_score(a.e_p + r0, q + wv * PH, vv + PH), s1 = 0.0f;
            if (two) s1 = attn_score(a.e_p + r1, q + wv * PH, vv + PH);
            const float l0 = vis0 ? -INFINITY : a.clip * d_tanhf(s0), l1 = vis1 ? -INFINITY : a.clip * d_tanhf(s1);
            const float mx = wave_max(vmax_raw(l0, l1));
            const float x0 = vis0 ? 0.0f : d_expf(l0 - mx), x1 = vis1 ? 0.0f : d_expf(l1 - mx);
            const float lse = d_logf(wave_tree_sum(x0 + x1));
            const float lp0 = vis0 ? -INFINITY : (l0 - mx) - lse, lp1 = vis1 ? -INFINITY : (l1 - mx) - lse;
            float k0 = lp0, k1 = lp1;
            if (mode == EAMRL_SAMPLE) {
                float z0, z1;
                if (use_rng) {
                    float nz[4];
                    exp1_noise4(seed, bi, t, n0 >> 2, nz);
                    z0 = nz[n0 & 3];
                    exp1_noise4(seed, bi, t, n1 >> 2, nz);
                    z1 = nz[n1 & 3];
                } else {
                    const float* nr = noise + ((size_t)bi * N + t) * N;
                    z0 = nr[in0 ? n0 : 0];
                    z1 = nr[in1 ? n1 : 0];
                }
                k0 = vis0 ? -INFINITY : d_expf(lp0) / z0;
                k1 = vis1 ? -INFINITY : d_expf(lp1) / z1;
            }
            float best = k0;
            int besti = n0;
            if (k1 > k0) { best = k1; besti = n1; }                 // first maximum: n0 < n1
            wave_argmax(best, besti);
            int sel = besti;
            if (mode == EAMRL_EVALUATE) sel = (int)given[(size_t)bi * N + t];
            sel = sel < 0 ? 0 : (sel >= N ? N - 1 : sel);             // a tour entry out of range reads node 0 / N - 1, never memory
            const float lps = __shfl((sel & 64) ? lp1 : lp0, sel & 63, 64);
            if (lane == 0) {
                if (bvalid) {
                    actions[(size_t)bi * N + t] = sel;
                    logp[(size_t)bi * N + t] = lps;
                }
                selxy[2 * wv] = xy[wv * (2 * NMAX) + 2 * sel];
                selxy[2 * wv + 1] = xy[wv * (2 * NMAX) + 2 * sel + 1];
            }
            vis0 = vis0 || n0 == sel;
            vis1 = vis1 || n1 == sel;
        }
        __syncthreads();
    }
}

}  // namespace

int launch_ptrnet_encode(const eamrl_ptrnet& p, hipStream_t st)
{
    if (p.B <= 0) return 0;
    hipLaunchKernelGGL(k_ptrnet_fold, dim3(PG / 256), dim3(256), 0, st, p.enc_w_ih, p.enc_b_ih, p.enc_b_hh, p.embedding,
                       (const float*)nullptr, p.ws + WS_ENC);
    hipLaunchKernelGGL(k_ptrnet_encode, dim3((unsigned)((p.B + ENC_TILE - 1) / ENC_TILE)), dim3(256), 0, st, p);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

int launch_ptrnet_rollout(const eamrl_ptrnet& p, int mode, const float* noise, const int64_t* given, int use_rng, uint64_t seed,
                          int64_t* actions, float* logp, hipStream_t st)
{
    if (p.B <= 0) return 0;
    hipLaunchKernelGGL(k_ptrnet_fold, dim3(PG / 256), dim3(256), 0, st, p.dec_w_ih, p.dec_b_ih, p.dec_b_hh, p.embedding,
                       p.dec_in0, p.ws + WS_DEC);
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_ptrnet_rollout), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)ROLLOUT_LDS) != hipSuccess)
            return EAMRL_E_LAUNCH;
        attr_set = true;
    }
    hipLaunchKernelGGL(k_ptrnet_rollout, dim3((unsigned)((p.B + DEC_TILE - 1) / DEC_TILE)), dim3(256), ROLLOUT_LDS, st, p, mode,
                       noise, given, use_rng, seed, actions, logp);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

}  // namespace eamrl
