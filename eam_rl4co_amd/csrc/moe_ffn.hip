// The MVMoE encoder's feed-forward sublayer: a sparsely gated mixture of experts (noisy top-k gating, 128 -> 512 -> 128 ReLU
// experts), as three launches on the caller's stream.
//
//   k_moe_gate      per row: gate logits, optional noise, softmax, top-k, gates; claims a slot in every chosen expert's row list
//                   (LDS counters per workgroup, one global integer atomic per expert and workgroup)
//   k_moe_experts   grouped GEMM: a workgroup takes four consecutive 16-row tiles of one expert's list, gathers the rows into LDS
//                   and runs both Linears on v_mfma_f32_16x16x4_f32, the hidden activations passing through LDS in 128-unit chunks
//   k_moe_combine   per row: y = sum over the selected experts in ascending expert index of g_e * o_e, the residual, and the
//                   optional BatchNorm1d(eval)
//
// Reference: rl4co/models/nn/moe.py:114-277 (MoE.noisy_top_k_gating, SparseDispatcher), wired into the encoder layer at
// rl4co/models/nn/graph/attnnet.py:38-42.
//
// Arithmetic (DESIGN.md "MoE encoder"; tests/moe_ref.py is the same statement on the CPU oracle), all float32, nothing contracted:
//   logit[e]  = chain_k(x[k], w_gate[k][e], 128, 0)                       (the k-ordered fma chain of eamrl_linear, no bias)
//   noisy:      std[e] = softplus(chain_k(x[k], w_noise[k][e])) + 1e-2f;  logit[e] = logit[e] + noise[row][e] * std[e]
//               softplus(v) = v > 20 ? v : d_logf(1 + d_expf(v))
//   p         = d_expf(logit - max) / (sum in ascending expert order)     (one correctly rounded division per expert)
//   selection = the k largest p, larger first, ties to the lower expert index
//   g[j]      = p[sel j] / (sum_j p[sel j] + 1e-6f)                       (sum in selection order)
//   o_e       = b2 + W2 relu(b1 + W1 x)                                   (both products the chain of eamrl_linear: the f32 MFMA
//                                                                          accumulates k in ascending order from the bias)
//   y         = 0; for the selected experts in ascending expert index: y = y + g_e * o_e   (unselected experts are skipped,
//               not multiplied by zero)
//   out       = [BN_eval](res + y)                                        (the epilogue of eamrl_linear_bn)
//
// The row lists are filled with integer atomics, so their order differs from run to run; every row's output is computed from
// that row alone, so values do not.  Grids depend on (rows, k, n_exp) only: the expert kernel runs the worst-case group count
// and its surplus workgroups leave after reading the counters.
#include "mfma_tile.hpp"

namespace eamrl {

constexpr int MOE_E = 128;           // embed_dim
constexpr int MOE_F = 512;           // expert hidden width
constexpr int MOE_MAXE = 8;          // experts
constexpr int MOE_CNT_BYTES = 64;    // 16 int32 counters at the head of the scratch

struct MoeArgs {
    const float* x;          // [rows][128]
    const float* w_gate;     // [128][n_exp]
    const float* w_noise;    // [128][n_exp] or NULL
    const float* noise;      // [rows][n_exp] or NULL
    const float* W1p;        // [n_exp][512 * 128] fragment order (eamrl_pack_linear_weight)
    const float* b1;         // [n_exp][512]
    const float* W2p;        // [n_exp][128 * 512] fragment order
    const float* b2;         // [n_exp][128]
    const float* res;        // [rows][128] or NULL
    const float* bn_gamma; const float* bn_beta; const float* bn_mean; const float* bn_var; float bn_eps;
    float* y;                // [rows][128]
    int8_t* sel;             // [rows][k]
    float* g;                // [rows][k]
    int32_t* cnt;            // [16]
    int32_t* list;           // [n_exp][rows]: row * 8 + selection slot
    float* o;                // [rows][k][128]
    int64_t rows; int n_exp, k;
    const int8_t* sel_in;    // [rows][k]: the caller's routing (eamrl_moe_experts_forward; `sel` is then its checked copy)
    int32_t* wgcnt;          // [ceil(rows / 256)][8]: the route kernels' per-workgroup counts, then list bases
};

// ---------------------------------------------------------------------------------------------------------------------------
// gate: 128 rows per workgroup, one thread per row; x staged through LDS in four 32-column chunks so the global reads coalesce
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int GR = 128, GC = 32, GCS = GC + 1;

__device__ __forceinline__ float moe_softplus(float v) { return v > 20.0f ? v : d_logf(1.0f + d_expf(v)); }

__global__ __launch_bounds__(GR) void k_moe_gate(MoeArgs a)
{
    __shared__ float XS[GR * GCS];
    __shared__ float WG[MOE_E * MOE_MAXE], WN[MOE_E * MOE_MAXE];
    __shared__ int lcnt[MOE_MAXE], lbase[MOE_MAXE];      // this workgroup's claims per expert, and where they start in the lists
    const int tid = threadIdx.x, ne = a.n_exp;
    if (tid < MOE_MAXE) lcnt[tid] = 0;
    const int64_t row0 = (int64_t)blockIdx.x * GR, row = row0 + tid;
    const bool noisy = a.noise != nullptr;
    for (int i = tid; i < MOE_E * ne; i += GR) {
        WG[i] = a.w_gate[i];
        WN[i] = noisy ? a.w_noise[i] : 0.0f;
    }
    float lg[MOE_MAXE], ln[MOE_MAXE];
#pragma unroll
    for (int e = 0; e < MOE_MAXE; ++e) lg[e] = ln[e] = 0.0f;
    for (int c0 = 0; c0 < MOE_E; c0 += GC) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < GC / 4; ++p) {
            const int f = tid + GR * p, r = f >> 3, q = f & 7;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row0 + r < a.rows) v = *reinterpret_cast<const float4*>(a.x + (row0 + r) * MOE_E + c0 + 4 * q);
            float* d = XS + r * GCS + 4 * q;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        __syncthreads();
        for (int c = 0; c < GC; ++c) {
            const float xv = XS[tid * GCS + c];
            const float* wg = WG + (c0 + c) * ne;
            const float* wn = WN + (c0 + c) * ne;
#pragma unroll
            for (int e = 0; e < MOE_MAXE; ++e)
                if (e < ne) {
                    lg[e] = fma_(xv, wg[e], lg[e]);
                    if (noisy) ln[e] = fma_(xv, wn[e], ln[e]);
                }
        }
    }
    const bool valid = row < a.rows;
    if (noisy && valid) {
#pragma unroll
        for (int e = 0; e < MOE_MAXE; ++e)
            if (e < ne) {
                const float sd = moe_softplus(ln[e]) + 1e-2f;
                const float nz = a.noise[row * ne + e] * sd;
                lg[e] = lg[e] + nz;
            }
    }
    float mx = lg[0];
#pragma unroll
    for (int e = 1; e < MOE_MAXE; ++e)
        if (e < ne && lg[e] > mx) mx = lg[e];
    float p[MOE_MAXE], sum = 0.0f;
#pragma unroll
    for (int e = 0; e < MOE_MAXE; ++e) {
        p[e] = e < ne ? d_expf(lg[e] - mx) : 0.0f;
        if (e < ne) sum = sum + p[e];
    }
#pragma unroll
    for (int e = 0; e < MOE_MAXE; ++e) p[e] = p[e] / sum;
    unsigned taken = 0;
    int se[MOE_MAXE];
    float sp[MOE_MAXE], tot = 0.0f;
#pragma unroll
    for (int j = 0; j < MOE_MAXE; ++j) {
        se[j] = 0; sp[j] = 0.0f;
        if (j < a.k) {
            int best = -1;
            float bv = 0.0f;
#pragma unroll
            for (int e = 0; e < MOE_MAXE; ++e)
                if (e < ne && !((taken >> e) & 1u) && (best < 0 || p[e] > bv)) { best = e; bv = p[e]; }
            taken |= 1u << best;
            se[j] = best; sp[j] = bv;
            tot = tot + bv;
        }
    }
    tot = tot + 1e-6f;
    // slots in the experts' row lists: claimed inside the workgroup on LDS counters, then one global atomic per expert and
    // workgroup (one global atomic per selection serialises on num_experts addresses: profiles/r18b_time_moe_global_claims.json)
    int lpos[MOE_MAXE];
#pragma unroll
    for (int j = 0; j < MOE_MAXE; ++j) {
        lpos[j] = 0;
        if (j < a.k && valid) {
            a.sel[row * a.k + j] = (int8_t)se[j];
            a.g[row * a.k + j] = sp[j] / tot;
            lpos[j] = atomicAdd(&lcnt[se[j]], 1);
        }
    }
    __syncthreads();
    if (tid < ne) lbase[tid] = atomicAdd(a.cnt + tid, lcnt[tid]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MOE_MAXE; ++j)
        if (j < a.k && valid)            // position < rows: a row names an expert at most once
            a.list[(int64_t)se[j] * a.rows + lbase[se[j]] + lpos[j]] = (int32_t)(row * 8 + j);
}

// ---------------------------------------------------------------------------------------------------------------------------
// experts: 256 threads take MRT consecutive 16-row tiles of one expert's list, so that every weight fragment fetched from L2
// serves MRT row tiles (one 16-row tile per workgroup re-read the expert's 512 KB of weights per tile and ran at the L2's
// pace: profiles/r18a_time_moe_16row_tiles.json).  The hidden
// activations pass through LDS in four chunks of 128 units, as in the fused encoder's FFN: chunk c of relu(b1 + W1 x) is
// written, then multiplied into the output accumulators, which stay in registers across the chunks -- k ascending over the 512
// hidden units, the chain of eamrl_linear.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int MRT = 4;                       // 16-row tiles per workgroup
constexpr int MROWS = 16 * MRT;
constexpr size_t MOE_EXPERT_LDS = (2 * MROWS * TS) * sizeof(float) + MROWS * sizeof(int);

// The tile products of the expert kernels, forward and backward: acc[rt][c] += (row tile rt of an A-layout LDS tile, 128 k-steps)
// x (the column tiles ct0 + c of a fragment-order pack that has kb 16-k blocks per column tile, its blocks u0 .. u0 + 7), k
// ascending.  `arow`: this lane's row of the tile (row j, k-group G); Wl: the pack + lane * 4.  WFIRST: the weights are the
// MFMA's first operand -- lane (j, G) of acc holds row j, columns 4 G + r of a column tile; otherwise its second -- column j,
// rows 4 G + r.  The backward recomputes the hidden activations through this very code: their bits, and so the ReLU mask,
// are the forward's.
template <bool WFIRST>
__device__ __forceinline__ void moe_tile_gemm(f32x4 (&acc)[MRT][2], const float* arow, const float* Wl, int ct0, int kb, int u0,
                                              int nrt)
{
#pragma unroll 2
    for (int u = 0; u < MOE_E / 16; ++u) {
        f32x4 w[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) w[c] = *reinterpret_cast<const f32x4*>(Wl + ((ct0 + c) * kb + u0 + u) * 256);
        float2 a0[MRT], a1[MRT];
#pragma unroll
        for (int rt = 0; rt < MRT; ++rt)
            if (rt < nrt) {
                a0[rt] = *reinterpret_cast<const float2*>(arow + rt * 16 * TS + 4 * u);
                a1[rt] = *reinterpret_cast<const float2*>(arow + rt * 16 * TS + 4 * u + 2);
            }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int rt = 0; rt < MRT; ++rt)
                if (rt < nrt) {
                    const float av = q == 0 ? a0[rt].x : q == 1 ? a0[rt].y : q == 2 ? a1[rt].x : a1[rt].y;
#pragma unroll
                    for (int c = 0; c < 2; ++c) acc[rt][c] = WFIRST ? mf(w[c][q], av, acc[rt][c]) : mf(av, w[c][q], acc[rt][c]);
                }
    }
}

// a wave's two column tiles of a 128-column chunk (lane (j, G): column j, rows 4 G + r) into an A-layout LDS tile; RELU: through
// the ReLU, as the forward stores its hidden chunk
template <bool RELU>
__device__ __forceinline__ void moe_tile_store(float* T, const f32x4 (&v)[MRT][2], int wv, int j, int G, int nrt)
{
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        float* d = T + a_off(16 * (2 * wv + c) + j);
#pragma unroll
        for (int rt = 0; rt < MRT; ++rt)
            if (rt < nrt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float t = v[rt][c][r];
                    d[(16 * rt + 4 * G + r) * TS] = RELU && !(t > 0.0f) ? 0.0f : t;
                }
            }
    }
}

// chunk ch of b1 + x W1^T (the hidden layer before its ReLU) of a group's rows: wave wv owns the chunk's column tiles 2 wv, 2 wv + 1
__device__ __forceinline__ void moe_hidden_chunk(f32x4 (&hid)[MRT][2], const float* xrow, const float* W1l, const float* b1, int ch,
                                                 int wv, int j, int nrt)
{
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float bj = b1[MOE_E * ch + 16 * (2 * wv + c) + j];
#pragma unroll
        for (int rt = 0; rt < MRT; ++rt) hid[rt][c] = (f32x4){bj, bj, bj, bj};
    }
    moe_tile_gemm<false>(hid, xrow, W1l, 8 * ch + 2 * wv, MOE_E / 16, 0, nrt);
}

// a workgroup's (expert, group of MROWS list rows) from the counters: false for the workgroups past the last group.  seg: the
// rows of the experts before e (the group's first row in list order is seg + MROWS * grp)
__device__ __forceinline__ bool moe_group_of(const int32_t* cnts, int n_exp, int b, int& e, int& grp, int& cnt, int& seg)
{
    e = -1; grp = 0; cnt = 0; seg = 0;
    int run = 0;
    for (int i = 0; i < n_exp; ++i) {
        const int c = cnts[i], t = (c + MROWS - 1) / MROWS;
        if (e < 0) {
            if (b < t) { e = i; grp = b; cnt = c; seg = run; }
            else b -= t;
        }
        run += c;
    }
    return e >= 0;
}

__global__ __launch_bounds__(256) void k_moe_experts(MoeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float moe_lds[];
    float* XA = moe_lds;                     // [MROWS][TS] gathered rows, A layout K = 128 (mfma_tile.hpp)
    float* HID = XA + MROWS * TS;            // [MROWS][TS] one 128-unit chunk of relu(b1 + W1 x), the same layout
    int* rowslot = reinterpret_cast<int*>(HID + MROWS * TS);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, G = lane >> 4;

    // this workgroup's (expert, group of MRT tiles) from the counters; workgroups past the last group leave
    int b = blockIdx.x, e = -1, grp = 0, cnt = 0;
    for (int i = 0; i < a.n_exp; ++i) {
        const int c = a.cnt[i], t = (c + MROWS - 1) / MROWS;
        if (e < 0) {
            if (b < t) { e = i; grp = b; cnt = c; }
            else b -= t;
        }
    }
    if (e < 0) return;
    const int n = cnt - MROWS * grp < MROWS ? cnt - MROWS * grp : MROWS;      // rows of this group, 1 .. MROWS
    const int nrt = __builtin_amdgcn_readfirstlane((n + 15) >> 4);            // its 16-row tiles; the list is read no further than n
    if (tid < MROWS) rowslot[tid] = tid < n ? a.list[(int64_t)e * a.rows + MROWS * grp + tid] : -1;
    __syncthreads();
#pragma unroll
    for (int p = 0; p < MROWS / 8; ++p) {
        const int f = tid + 256 * p, r = f >> 5, q4 = f & 31;
        const int rs = rowslot[r];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                 // padded rows: zeros, their results are never stored
        if (rs >= 0) v = *reinterpret_cast<const float4*>(a.x + (int64_t)(rs >> 3) * MOE_E + 4 * q4);
        float* d = XA + r * TS + q4;
        d[0] = v.x; d[TG] = v.y; d[2 * TG] = v.z; d[3 * TG] = v.w;
    }

    // output accumulators, weights as the MFMA's A operand: wave wv owns output column tiles 2 wv, 2 wv + 1; lane (j, G) holds
    // row j of a row tile and columns 4 G .. 4 G + 3 of a column tile (one 16-byte store)
    const float* W1 = a.W1p + (int64_t)e * (MOE_F * MOE_E) + lane * 4;
    const float* W2 = a.W2p + (int64_t)e * (MOE_E * MOE_F) + lane * 4;
    const float* b1 = a.b1 + e * MOE_F;
    const float* b2 = a.b2 + e * MOE_E;
    f32x4 out[MRT][2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float4 bq = *reinterpret_cast<const float4*>(b2 + 16 * (2 * wv + c) + 4 * G);
#pragma unroll
        for (int rt = 0; rt < MRT; ++rt) out[rt][c] = (f32x4){bq.x, bq.y, bq.z, bq.w};
    }
    const float* xrow = XA + j * TS + G * TG;
    const float* hrow = HID + j * TS + G * TG;
    __syncthreads();

    for (int ch = 0; ch < MOE_F / MOE_E; ++ch) {
        // hidden chunk = relu(b1 + x W1^T), units 128 ch .. 128 ch + 127: wave wv owns the chunk's column tiles 2 wv, 2 wv + 1;
        // lane (j, G): column j, rows 4 G + r of a row tile
        f32x4 hid[MRT][2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float bj = b1[MOE_E * ch + 16 * (2 * wv + c) + j];
#pragma unroll
            for (int rt = 0; rt < MRT; ++rt) hid[rt][c] = (f32x4){bj, bj, bj, bj};
        }
#pragma unroll 2
        for (int u = 0; u < MOE_E / 16; ++u) {
            f32x4 w[2];
#pragma unroll
            for (int c = 0; c < 2; ++c)
                w[c] = *reinterpret_cast<const f32x4*>(W1 + ((8 * ch + 2 * wv + c) * (MOE_E / 16) + u) * 256);
            float2 a0[MRT], a1[MRT];
#pragma unroll
            for (int rt = 0; rt < MRT; ++rt)
                if (rt < nrt) {
                    a0[rt] = *reinterpret_cast<const float2*>(xrow + rt * 16 * TS + 4 * u);
                    a1[rt] = *reinterpret_cast<const float2*>(xrow + rt * 16 * TS + 4 * u + 2);
                }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int rt = 0; rt < MRT; ++rt)
                    if (rt < nrt) {
                        const float av = q == 0 ? a0[rt].x : q == 1 ? a0[rt].y : q == 2 ? a1[rt].x : a1[rt].y;
#pragma unroll
                        for (int c = 0; c < 2; ++c) hid[rt][c] = mf(av, w[c][q], hid[rt][c]);
                    }
        }
        if (ch) __syncthreads();            // the previous chunk has been multiplied: HID is free
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int col = 16 * (2 * wv + c) + j;
            float* d = HID + a_off(col);
#pragma unroll
            for (int rt = 0; rt < MRT; ++rt)
                if (rt < nrt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = hid[rt][c][r];
                        d[(16 * rt + 4 * G + r) * TS] = !(v > 0.0f) ? 0.0f : v;
                    }
                }
        }
        __syncthreads();
        // out += hidden chunk x W2^T over k = 128 ch .. 128 ch + 127
#pragma unroll 2
        for (int u = 0; u < MOE_E / 16; ++u) {
            f32x4 w[2];
#pragma unroll
            for (int c = 0; c < 2; ++c)
                w[c] = *reinterpret_cast<const f32x4*>(W2 + ((2 * wv + c) * (MOE_F / 16) + 8 * ch + u) * 256);
            float2 a0[MRT], a1[MRT];
#pragma unroll
            for (int rt = 0; rt < MRT; ++rt)
                if (rt < nrt) {
                    a0[rt] = *reinterpret_cast<const float2*>(hrow + rt * 16 * TS + 4 * u);
                    a1[rt] = *reinterpret_cast<const float2*>(hrow + rt * 16 * TS + 4 * u + 2);
                }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int rt = 0; rt < MRT; ++rt)
                    if (rt < nrt) {
                        const float av = q == 0 ? a0[rt].x : q == 1 ? a0[rt].y : q == 2 ? a1[rt].x : a1[rt].y;
#pragma unroll
                        for (int c = 0; c < 2; ++c) out[rt][c] = mf(w[c][q], av, out[rt][c]);
                    }
        }
    }
#pragma unroll
    for (int rt = 0; rt < MRT; ++rt)
        if (rt < nrt) {
            const int rs = rowslot[16 * rt + j];
            if (rs >= 0) {
                float* op = a.o + ((int64_t)(rs >> 3) * a.k + (rs & 7)) * MOE_E + 4 * G;
#pragma unroll
                for (int c = 0; c < 2; ++c)
                    *reinterpret_cast<float4*>(op + 16 * (2 * wv + c)) =
                        make_float4(out[rt][c][0], out[rt][c][1], out[rt][c][2], out[rt][c][3]);
            }
        }
}

// The same kernel written on the shared tile functions above, for the training graph (eamrl_moe_experts_forward): its hidden
// chunk is moe_hidden_chunk, which the backward calls again, so the backward's ReLU mask is this forward's.  Per accumulator the
// MFMA sequence is k_moe_experts', and tests/test_gpu_moe_backward.py holds the two to the same bits.  k_moe_experts itself is
// kept as it was: built from these functions the compiler allocates it differently (68 VGPRs against 80) and the rollout's
// sublayer measured 0.695 ms against 0.650 ms at 103 424 rows (tools/time_moe.py, separate processes).
__global__ __launch_bounds__(256) void k_moe_experts_train(MoeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float moe_lds[];
    float* XA = moe_lds;                     // [MROWS][TS] gathered rows, A layout K = 128 (mfma_tile.hpp)
    float* HID = XA + MROWS * TS;            // [MROWS][TS] one 128-unit chunk of relu(b1 + W1 x), the same layout
    int* rowslot = reinterpret_cast<int*>(HID + MROWS * TS);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, G = lane >> 4;

    // this workgroup's (expert, group of MRT tiles) from the counters; workgroups past the last group leave
    int e, grp, cnt, seg;
    if (!moe_group_of(a.cnt, a.n_exp, blockIdx.x, e, grp, cnt, seg)) return;
    const int n = cnt - MROWS * grp < MROWS ? cnt - MROWS * grp : MROWS;      // rows of this group, 1 .. MROWS
    const int nrt = __builtin_amdgcn_readfirstlane((n + 15) >> 4);            // its 16-row tiles; the list is read no further than n
    if (tid < MROWS) rowslot[tid] = tid < n ? a.list[(int64_t)e * a.rows + MROWS * grp + tid] : -1;
    __syncthreads();
#pragma unroll
    for (int p = 0; p < MROWS / 8; ++p) {
        const int f = tid + 256 * p, r = f >> 5, q4 = f & 31;
        const int rs = rowslot[r];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                 // padded rows: zeros, their results are never stored
        if (rs >= 0) v = *reinterpret_cast<const float4*>(a.x + (int64_t)(rs >> 3) * MOE_E + 4 * q4);
        float* d = XA + r * TS + q4;
        d[0] = v.x; d[TG] = v.y; d[2 * TG] = v.z; d[3 * TG] = v.w;
    }

    // output accumulators, weights as the MFMA's A operand: wave wv owns output column tiles 2 wv, 2 wv + 1; lane (j, G) holds
    // row j of a row tile and columns 4 G .. 4 G + 3 of a column tile (one 16-byte store)
    const float* W1 = a.W1p + (int64_t)e * (MOE_F * MOE_E) + lane * 4;
    const float* W2 = a.W2p + (int64_t)e * (MOE_E * MOE_F) + lane * 4;
    const float* b1 = a.b1 + e * MOE_F;
    const float* b2 = a.b2 + e * MOE_E;
    f32x4 out[MRT][2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float4 bq = *reinterpret_cast<const float4*>(b2 + 16 * (2 * wv + c) + 4 * G);
#pragma unroll
        for (int rt = 0; rt < MRT; ++rt) out[rt][c] = (f32x4){bq.x, bq.y, bq.z, bq.w};
    }
    const float* xrow = XA + j * TS + G * TG;
    const float* hrow = HID + j * TS + G * TG;
    __syncthreads();

    for (int ch = 0; ch < MOE_F / MOE_E; ++ch) {
        // hidden chunk = relu(b1 + x W1^T), units 128 ch .. 128 ch + 127: wave wv owns the chunk's column tiles 2 wv, 2 wv + 1;
        // lane (j, G): column j, rows 4 G + r of a row tile
        f32x4 hid[MRT][2];
        moe_hidden_chunk(hid, xrow, W1, b1, ch, wv, j, nrt);
        if (ch) __syncthreads();            // the previous chunk has been multiplied: HID is free
        moe_tile_store<true>(HID, hid, wv, j, G, nrt);
        __syncthreads();
        // out += hidden chunk x W2^T over k = 128 ch .. 128 ch + 127
        moe_tile_gemm<true>(out, hrow, W2, 2 * wv, MOE_F / 16, 8 * ch, nrt);
    }
#pragma unroll
    for (int rt = 0; rt < MRT; ++rt)
        if (rt < nrt) {
            const int rs = rowslot[16 * rt + j];
            if (rs >= 0) {
                float* op = a.o + ((int64_t)(rs >> 3) * a.k + (rs & 7)) * MOE_E + 4 * G;
#pragma unroll
                for (int c = 0; c < 2; ++c)
                    *reinterpret_cast<float4*>(op + 16 * (2 * wv + c)) =
                        make_float4(out[rt][c][0], out[rt][c][1], out[rt][c][2], out[rt][c][3]);
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------------------
// combine: 32 threads per row, four columns each
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_moe_combine(MoeArgs a)
{
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, row = gid >> 5;
    const int c4 = (int)(gid & 31) * 4;
    if (row >= a.rows) return;
    float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int e = 0; e < a.n_exp; ++e)
        for (int s = 0; s < a.k; ++s)
            if (a.sel[row * a.k + s] == e) {
                const float gv = a.g[row * a.k + s];
                const float4 o4 = *reinterpret_cast<const float4*>(a.o + (row * a.k + s) * MOE_E + c4);
                const float ov[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float t = gv * ov[q];
                    y[q] = y[q] + t;
                }
            }
    if (a.res) {
        const float4 r4 = *reinterpret_cast<const float4*>(a.res + row * MOE_E + c4);
        y[0] = r4.x + y[0]; y[1] = r4.y + y[1]; y[2] = r4.z + y[2]; y[3] = r4.w + y[3];
    }
    if (a.bn_gamma) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {       // eamrl_linear_bn's per-column constants and epilogue
            const int c = c4 + q;
            const float scale = a.bn_gamma[c] / __builtin_sqrtf(a.bn_var[c] + a.bn_eps);
            const float ms = a.bn_mean[c] * scale;
            y[q] = fma_(y[q], scale, a.bn_beta[c] - ms);
        }
    }
    *reinterpret_cast<float4*>(a.y + row * MOE_E + c4) = make_float4(y[0], y[1], y[2], y[3]);
}

// counters | lists (n_exp * rows int32, padded to 16 bytes) | o (rows * k * 128 floats)
static int64_t moe_list_bytes(int64_t rows, int n_exp) { return 16 * ((rows * n_exp + 3) / 4); }

bool moe_ffn_supports(int64_t rows, int E, int F, int n_exp, int k)
{
    return rows >= 0 && rows <= (int64_t)1 << 24 && E == MOE_E && F == MOE_F && n_exp >= 1 && n_exp <= MOE_MAXE && k >= 1 && k <= n_exp;
}

int64_t moe_ffn_scratch_bytes(int64_t rows, int n_exp, int k)
{
    if (!moe_ffn_supports(rows, MOE_E, MOE_F, n_exp, k)) return -1;
    return MOE_CNT_BYTES + moe_list_bytes(rows, n_exp) + 4 * rows * k * MOE_E;
}

// the grouped expert GEMM over the lists in a.cnt / a.list (train: k_moe_experts_train), then the combine
static int launch_experts_and_combine(const MoeArgs& a, bool train, hipStream_t st)
{
    static_assert(MOE_EXPERT_LDS <= 80 * 1024, "two expert workgroups per CU");
    static const bool lds_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(k_moe_experts),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)MOE_EXPERT_LDS) == hipSuccess &&
                               hipFuncSetAttribute(reinterpret_cast<const void*>(k_moe_experts_train),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)MOE_EXPERT_LDS) == hipSuccess;
    if (!lds_ok) return EAMRL_E_LAUNCH;
    const int64_t groups = (a.rows * a.k + MROWS - 1) / MROWS + a.n_exp;      // every expert's list may end in a partial group
    hipLaunchKernelGGL(train ? k_moe_experts_train : k_moe_experts, dim3((unsigned)groups), dim3(256), MOE_EXPERT_LDS, st, a);
    hipLaunchKernelGGL(k_moe_combine, dim3((unsigned)((a.rows * 32 + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

int launch_moe_ffn(const eamrl_moe_layer& m, hipStream_t st)
{
    const int64_t rows = m.rows;
    if (rows == 0) return 0;
    MoeArgs a = {};
    a.x = m.x; a.w_gate = m.w_gate; a.w_noise = m.noise ? m.w_noise : nullptr; a.noise = m.noise;
    a.W1p = m.W1p; a.b1 = m.b1; a.W2p = m.W2p; a.b2 = m.b2; a.res = m.res;
    a.bn_gamma = m.bn_gamma; a.bn_beta = m.bn_beta; a.bn_mean = m.bn_mean; a.bn_var = m.bn_var; a.bn_eps = m.bn_eps;
    a.y = m.y; a.sel = m.sel; a.g = m.g;
    char* s = static_cast<char*>(m.scratch);
    a.cnt = reinterpret_cast<int32_t*>(s);
    a.list = reinterpret_cast<int32_t*>(s + MOE_CNT_BYTES);
    a.o = reinterpret_cast<float*>(s + MOE_CNT_BYTES + moe_list_bytes(rows, m.n_exp));
    a.rows = rows; a.n_exp = m.n_exp; a.k = m.k;
    if (hipMemsetAsync(a.cnt, 0, MOE_CNT_BYTES, st) != hipSuccess) return EAMRL_E_LAUNCH;
    hipLaunchKernelGGL(k_moe_gate, dim3((unsigned)((rows + GR - 1) / GR)), dim3(GR), 0, st, a);
    return launch_experts_and_combine(a, false, st);
}

// ===========================================================================================================================
// The experts on a GIVEN routing and their backward (eamrl_moe_experts_forward / _backward): the training graph's sparse half.
//
// forward    k_moe_route_count / _scan / _fill   the experts' row lists in ascending row order: per-workgroup counts, an exclusive
//                                                scan over the workgroups, then every row's position = its workgroup's base + its
//                                                rank among the workgroup's rows (wave ballots).  Nothing depends on scheduling, so
//                                                the weight gradients, which sum over a list, repeat bit for bit.
//            k_moe_experts_train, k_moe_combine  the expert kernel on the shared tile functions, the combine as above
// backward   k_moe_experts_bwd                   per 64-row group of one expert: gathers x and dO = g * dy, then per 128-unit chunk
//                                                recomputes hid (moe_hidden_chunk, the forward's code), dHid = (dO W2) * [hid > 0]
//                                                on the pack of W2^T, and dX += dHid W1 on the pack of W1^T; writes x, dO, hid,
//                                                dHid in list order ("compact": every expert's rows are one contiguous segment)
//                                                and dX per (row, slot)
//            k_grouped_wgrad + k_wgrad_reduce    (train_gemm.hip) dW2 = dO^T hid, dW1 = dHid^T x and the bias sums per segment
//            k_moe_bwd_rows                      per row: dg[j] = <dy, o_j>, dx = the slots' dX in ascending expert index
// ===========================================================================================================================
constexpr int RR = 256;              // rows per route workgroup

// a row's routing as one nibble per expert: (the first slot naming expert e) + 1, or 0.  Entries outside 0 .. n_exp - 1 and
// repeated ones are dropped and counted in `bad`.
__device__ __forceinline__ unsigned route_row(const int8_t* sel_in, int64_t row, int k, int n_exp, int& bad)
{
    unsigned sw = 0;
    bad = 0;
    for (int j = 0; j < k; ++j) {
        const int e = sel_in[row * k + j];
        if (e < 0 || e >= n_exp || ((sw >> (4 * e)) & 15u)) ++bad;
        else sw |= (unsigned)(j + 1) << (4 * e);
    }
    return sw;
}

__global__ __launch_bounds__(RR) void k_moe_route_count(MoeArgs a)
{
    __shared__ int wc[RR / 64][MOE_MAXE];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t row = (int64_t)blockIdx.x * RR + tid;
    int bad = 0;
    const unsigned sw = row < a.rows ? route_row(a.sel_in, row, a.k, a.n_exp, bad) : 0u;
    for (int e = 0; e < a.n_exp; ++e) {
        const unsigned long long m = __ballot(((sw >> (4 * e)) & 15u) != 0);
        if (lane == 0) wc[wv][e] = __popcll(m);
    }
    if (bad) atomicAdd(a.cnt + 15, bad);            // an integer count: the order of the additions does not show
    __syncthreads();
    if (tid < a.n_exp) a.wgcnt[(int64_t)blockIdx.x * MOE_MAXE + tid] = (wc[0][tid] + wc[1][tid]) + (wc[2][tid] + wc[3][tid]);
}

// one workgroup: per expert, the exclusive scan of the nwg workgroup counts (in place: counts become list bases) and the total
__global__ __launch_bounds__(256) void k_moe_route_scan(MoeArgs a, int nwg)
{
    __shared__ int part[256];
    const int tid = threadIdx.x, per = (nwg + 255) / 256;
    const int b0 = tid * per < nwg ? tid * per : nwg, b1 = b0 + per < nwg ? b0 + per : nwg;
    for (int e = 0; e < a.n_exp; ++e) {
        int s = 0;
        for (int b = b0; b < b1; ++b) s += a.wgcnt[(int64_t)b * MOE_MAXE + e];
        part[tid] = s;
        __syncthreads();
        int base = 0;
        for (int t = 0; t < tid; ++t) base += part[t];
        for (int b = b0; b < b1; ++b) {
            const int c = a.wgcnt[(int64_t)b * MOE_MAXE + e];
            a.wgcnt[(int64_t)b * MOE_MAXE + e] = base;
            base += c;
        }
        if (tid == 255) a.cnt[e] = base;
        __syncthreads();
    }
}

__global__ __launch_bounds__(RR) void k_moe_route_fill(MoeArgs a)
{
    __shared__ int wc[RR / 64][MOE_MAXE];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t row = (int64_t)blockIdx.x * RR + tid;
    int bad = 0;
    const unsigned sw = row < a.rows ? route_row(a.sel_in, row, a.k, a.n_exp, bad) : 0u;
    const unsigned long long below = (1ull << lane) - 1ull;
    int rk[MOE_MAXE];
#pragma unroll
    for (int e = 0; e < MOE_MAXE; ++e) {
        rk[e] = 0;
        if (e < a.n_exp) {
            const unsigned long long m = __ballot(((sw >> (4 * e)) & 15u) != 0);
            rk[e] = __popcll(m & below);
            if (lane == 0) wc[wv][e] = __popcll(m);
        }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < MOE_MAXE; ++e)
        if (e < a.n_exp) {
            const int slot1 = (int)((sw >> (4 * e)) & 15u);
            if (slot1) {           // position < rows: a row is listed by an expert at most once
                int pos = a.wgcnt[(int64_t)blockIdx.x * MOE_MAXE + e] + rk[e];
                for (int w = 0; w < wv; ++w) pos += wc[w][e];
                a.list[(int64_t)e * a.rows + pos] = (int32_t)(row * 8 + slot1 - 1);
            }
        }
    if (row < a.rows)
        for (int j = 0; j < a.k; ++j) {
            const int e = a.sel_in[row * a.k + j];
            const bool ok = e >= 0 && e < a.n_exp && (int)((sw >> (4 * e)) & 15u) == j + 1;
            a.sel[row * a.k + j] = (int8_t)(ok ? e : -1);
        }
}

struct MoeBwdArgs {
    const float* x;          // [rows][128]
    const float* dy;         // [rows][128]
    const float* g;          // [rows][k]
    const float* W1p; const float* b1;       // the forward's pack of W1 and its bias
    const float* W2Tp;       // [n_exp][512 * 128]: pack of W2^T [512][128]
    const float* W1Tp;       // [n_exp][128 * 512]: pack of W1^T [128][512]
    const int8_t* sel;       // [rows][k] checked (dropped entries -1)
    const float* o;          // [rows][k][128]
    const int32_t* cnt; const int32_t* list;
    float* Xc; float* dOc;   // [rows * k][128] in list order, or NULL: no weight gradients
    float* Hc; float* dHc;   // [rows * k][512]
    float* dxs;              // [rows][k][128] per-slot dX, or NULL: no input gradient
    float* dx;               // [rows][128] or NULL
    float* dg;               // [rows][k] or NULL
    int64_t rows; int n_exp, k;
};

constexpr size_t MOE_BWD_LDS = (3 * MROWS * TS) * sizeof(float) + MROWS * sizeof(int);

__global__ __launch_bounds__(256) void k_moe_experts_bwd(MoeBwdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float moe_lds[];
    float* XA = moe_lds;                     // [MROWS][TS] gathered x rows, A layout
    float* DO = XA + MROWS * TS;             // [MROWS][TS] gathered g * dy rows
    float* DH = DO + MROWS * TS;             // [MROWS][TS] one 128-unit chunk of dHid
    int* rowslot = reinterpret_cast<int*>(DH + MROWS * TS);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, G = lane >> 4;

    int e, grp, cnt, seg;
    if (!moe_group_of(a.cnt, a.n_exp, blockIdx.x, e, grp, cnt, seg)) return;
    const int n = cnt - MROWS * grp < MROWS ? cnt - MROWS * grp : MROWS;
    const int nrt = __builtin_amdgcn_readfirstlane((n + 15) >> 4);
    const int64_t base = (int64_t)seg + MROWS * grp;            // the group's first row in list order (< rows * k)
    const bool wgrads = a.Xc != nullptr, dxs = a.dxs != nullptr;
    if (tid < MROWS) rowslot[tid] = tid < n ? a.list[(int64_t)e * a.rows + MROWS * grp + tid] : -1;
    __syncthreads();
#pragma unroll
    for (int p = 0; p < MROWS / 8; ++p) {
        const int f = tid + 256 * p, r = f >> 5, q4 = f & 31;
        const int rs = rowslot[r];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f), d = v;          // padded rows: zeros, their results are never stored
        if (rs >= 0) {
            const int64_t row = rs >> 3;
            v = *reinterpret_cast<const float4*>(a.x + row * MOE_E + 4 * q4);
            d = *reinterpret_cast<const float4*>(a.dy + row * MOE_E + 4 * q4);
            const float gv = a.g[row * a.k + (rs & 7)];
            d.x = gv * d.x; d.y = gv * d.y; d.z = gv * d.z; d.w = gv * d.w;
            if (wgrads) {
                *reinterpret_cast<float4*>(a.Xc + (base + r) * MOE_E + 4 * q4) = v;
                *reinterpret_cast<float4*>(a.dOc + (base + r) * MOE_E + 4 * q4) = d;
            }
        }
        float* xd = XA + r * TS + q4;
        xd[0] = v.x; xd[TG] = v.y; xd[2 * TG] = v.z; xd[3 * TG] = v.w;
        float* dd = DO + r * TS + q4;
        dd[0] = d.x; dd[TG] = d.y; dd[2 * TG] = d.z; dd[3 * TG] = d.w;
    }
    const float* W1 = a.W1p + (int64_t)e * (MOE_F * MOE_E) + lane * 4;
    const float* W2T = a.W2Tp + (int64_t)e * (MOE_F * MOE_E) + lane * 4;
    const float* W1T = a.W1Tp + (int64_t)e * (MOE_E * MOE_F) + lane * 4;
    const float* b1 = a.b1 + e * MOE_F;
    f32x4 dxa[MRT][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int rt = 0; rt < MRT; ++rt) dxa[rt][c] = z4();
    const float* xrow = XA + j * TS + G * TG;
    const float* dorow = DO + j * TS + G * TG;
    const float* dhrow = DH + j * TS + G * TG;
    __syncthreads();

    for (int ch = 0; ch < MOE_F / MOE_E; ++ch) {
        // hid and dHid of the chunk in the same lane layout: column j of the wave's column tiles, rows 4 G + r
        f32x4 hid[MRT][2], dh[MRT][2];
        moe_hidden_chunk(hid, xrow, W1, b1, ch, wv, j, nrt);
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int rt = 0; rt < MRT; ++rt) dh[rt][c] = z4();
        moe_tile_gemm<false>(dh, dorow, W2T, 8 * ch + 2 * wv, MOE_E / 16, 0, nrt);
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int rt = 0; rt < MRT; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (!(hid[rt][c][r] > 0.0f)) hid[rt][c][r] = dh[rt][c][r] = 0.0f;          // the forward's ReLU and its mask
        if (wgrads) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int col = MOE_E * ch + 16 * (2 * wv + c) + j;
#pragma unroll
                for (int rt = 0; rt < MRT; ++rt)
                    if (rt < nrt) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int lr = 16 * rt + 4 * G + r;
                            if (lr < n) {
                                a.Hc[(base + lr) * MOE_F + col] = hid[rt][c][r];
                                a.dHc[(base + lr) * MOE_F + col] = dh[rt][c][r];
                            }
                        }
                    }
            }
        }
        if (dxs) {
            if (ch) __syncthreads();            // the previous chunk has been multiplied: DH is free
            moe_tile_store<false>(DH, dh, wv, j, G, nrt);
            __syncthreads();
            // dX += dHid chunk x W1 over the units 128 ch .. 128 ch + 127
            moe_tile_gemm<true>(dxa, dhrow, W1T, 2 * wv, MOE_F / 16, 8 * ch, nrt);
        }
    }
    if (dxs) {
#pragma unroll
        for (int rt = 0; rt < MRT; ++rt)
            if (rt < nrt) {
                const int rs = rowslot[16 * rt + j];
                if (rs >= 0) {
                    float* op = a.dxs + ((int64_t)(rs >> 3) * a.k + (rs & 7)) * MOE_E + 4 * G;
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        *reinterpret_cast<float4*>(op + 16 * (2 * wv + c)) =
                            make_float4(dxa[rt][c][0], dxa[rt][c][1], dxa[rt][c][2], dxa[rt][c][3]);
                }
            }
    }
}

// per row, 32 threads with four columns each: dg[j] = <dy, o_j> (partner sums in a fixed order), dx = the slots' dX in ascending
// expert index; a dropped slot (sel -1) has dg = 0 and no dX
__global__ __launch_bounds__(256) void k_moe_bwd_rows(MoeBwdArgs a)
{
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid >> 5 < a.rows ? gid >> 5 : a.rows - 1;     // (the last workgroup's spare rows repeat the last row)
    const bool live = gid >> 5 < a.rows;
    const int c4 = (int)(gid & 31) * 4;
    if (a.dg) {
        const float4 d4 = *reinterpret_cast<const float4*>(a.dy + row * MOE_E + c4);
        for (int s = 0; s < a.k; ++s) {
            float v = 0.0f;
            if (a.sel[row * a.k + s] >= 0) {
                const float4 o4 = *reinterpret_cast<const float4*>(a.o + (row * a.k + s) * MOE_E + c4);
                v = (d4.x * o4.x + d4.y * o4.y) + (d4.z * o4.z + d4.w * o4.w);
            }
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 8, 64);
            v += __shfl_xor(v, 4, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 1, 64);
            if (live && c4 == 0) a.dg[row * a.k + s] = v;
        }
    }
    if (a.dx && live) {
        float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int e = 0; e < a.n_exp; ++e)
            for (int s = 0; s < a.k; ++s)
                if (a.sel[row * a.k + s] == e) {
                    const float4 t = *reinterpret_cast<const float4*>(a.dxs + (row * a.k + s) * MOE_E + c4);
                    y[0] = y[0] + t.x; y[1] = y[1] + t.y; y[2] = y[2] + t.z; y[3] = y[3] + t.w;
                }
        *reinterpret_cast<float4*>(a.dx + row * MOE_E + c4) = make_float4(y[0], y[1], y[2], y[3]);
    }
}

// state: counters | lists | o | checked sel (padded to 16 bytes) | per-workgroup counts (8 int32 per 256 rows)
struct MoeState { int32_t* cnt; int32_t* list; float* o; int8_t* sel; int32_t* wgcnt; };
static int64_t moe_sel_bytes(int64_t rows, int k) { return 16 * ((rows * k + 15) / 16); }
static MoeState moe_state(void* p, int64_t rows, int n_exp, int k)
{
    char* s = static_cast<char*>(p);
    MoeState t;
    t.cnt = reinterpret_cast<int32_t*>(s);
    t.list = reinterpret_cast<int32_t*>(s + MOE_CNT_BYTES);
    s += MOE_CNT_BYTES + moe_list_bytes(rows, n_exp);
    t.o = reinterpret_cast<float*>(s);
    s += 4 * rows * k * MOE_E;
    t.sel = reinterpret_cast<int8_t*>(s);
    t.wgcnt = reinterpret_cast<int32_t*>(s + moe_sel_bytes(rows, k));
    return t;
}

int64_t moe_experts_state_bytes(int64_t rows, int n_exp, int k)
{
    if (!moe_ffn_supports(rows, MOE_E, MOE_F, n_exp, k)) return -1;
    return MOE_CNT_BYTES + moe_list_bytes(rows, n_exp) + 4 * rows * k * MOE_E + moe_sel_bytes(rows, k) +
           4 * MOE_MAXE * ((rows + RR - 1) / RR);
}

// compact x, dO [T][128], hid, dHid [T][512], per-slot dX [T][128] (T = rows * k), then the weight gradients' partial blocks
// (one buffer: the two gradients run one after the other on the stream)
int64_t moe_experts_bwd_scratch_bytes(int64_t rows, int n_exp, int k)
{
    if (!moe_ffn_supports(rows, MOE_E, MOE_F, n_exp, k)) return -1;
    const int64_t T = rows * k;
    return 4 * (T * (3 * MOE_E + 2 * MOE_F) + grouped_wgrad_scratch(T, n_exp, MOE_F, MOE_E));     // (dW1's blocks carry 512 db)
}

int launch_moe_experts_forward(const eamrl_moe_experts& m, hipStream_t st)
{
    const int64_t rows = m.rows;
    if (rows == 0) return 0;
    const MoeState t = moe_state(m.state, rows, m.n_exp, m.k);
    MoeArgs a = {};
    a.x = m.x; a.W1p = m.W1p; a.b1 = m.b1; a.W2p = m.W2p; a.b2 = m.b2;
    a.y = m.y; a.sel_in = m.sel; a.sel = t.sel; a.g = const_cast<float*>(m.g);      // (read only on this path)
    a.cnt = t.cnt; a.list = t.list; a.o = t.o; a.wgcnt = t.wgcnt;
    a.rows = rows; a.n_exp = m.n_exp; a.k = m.k;
    if (hipMemsetAsync(a.cnt, 0, MOE_CNT_BYTES, st) != hipSuccess) return EAMRL_E_LAUNCH;
    const int nwg = (int)((rows + RR - 1) / RR);
    hipLaunchKernelGGL(k_moe_route_count, dim3(nwg), dim3(RR), 0, st, a);
    hipLaunchKernelGGL(k_moe_route_scan, dim3(1), dim3(256), 0, st, a, nwg);
    hipLaunchKernelGGL(k_moe_route_fill, dim3(nwg), dim3(RR), 0, st, a);
    return launch_experts_and_combine(a, true, st);
}

int launch_moe_experts_backward(const eamrl_moe_experts& m, hipStream_t st)
{
    const int64_t rows = m.rows, T = rows * m.k;
    if (rows == 0) return 0;
    const MoeState t = moe_state(m.state, rows, m.n_exp, m.k);
    MoeBwdArgs a = {};
    a.x = m.x; a.dy = m.dy; a.g = m.g; a.W1p = m.W1p; a.b1 = m.b1; a.W2Tp = m.W2Tp; a.W1Tp = m.W1Tp;
    a.sel = t.sel; a.o = t.o; a.cnt = t.cnt; a.list = t.list;
    float* s = static_cast<float*>(m.scratch);
    float* part = s + T * (3 * MOE_E + 2 * MOE_F);
    if (m.dW1) {
        a.Xc = s; a.dOc = s + T * MOE_E; a.Hc = s + 2 * T * MOE_E; a.dHc = a.Hc + T * MOE_F;
    }
    if (m.dx) a.dxs = s + T * (2 * MOE_E + 2 * MOE_F);
    a.dx = m.dx; a.dg = m.dg;
    a.rows = rows; a.n_exp = m.n_exp; a.k = m.k;
    if (m.dW1 || m.dx) {
        static const bool lds_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(k_moe_experts_bwd),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)MOE_BWD_LDS) == hipSuccess;
        if (!lds_ok) return EAMRL_E_LAUNCH;
        const int64_t groups = (T + MROWS - 1) / MROWS + m.n_exp;
        hipLaunchKernelGGL(k_moe_experts_bwd, dim3((unsigned)groups), dim3(256), MOE_BWD_LDS, st, a);
    }
    if (m.dW1) {
        if (launch_grouped_wgrad(a.dOc, MOE_E, a.Hc, MOE_F, T, a.cnt, m.n_exp, MOE_E, MOE_F, m.dW2, m.db2, part, st)) return EAMRL_E_LAUNCH;
        if (launch_grouped_wgrad(a.dHc, MOE_F, a.Xc, MOE_E, T, a.cnt, m.n_exp, MOE_F, MOE_E, m.dW1, m.db1, part, st)) return EAMRL_E_LAUNCH;
    }
    if (m.dx || m.dg) hipLaunchKernelGGL(k_moe_bwd_rows, dim3((unsigned)((rows * 32 + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

}  // namespace eamrl
