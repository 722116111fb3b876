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
    static_assert(MOE_EXPERT_LDS <= 80 * 1024, "two expert workgroups per CU");
    static const bool lds_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(k_moe_experts),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)MOE_EXPERT_LDS) == hipSuccess;
    if (!lds_ok) return EAMRL_E_LAUNCH;
    const int64_t groups = (rows * m.k + MROWS - 1) / MROWS + m.n_exp;      // every expert's list may end in a partial group
    hipLaunchKernelGGL(k_moe_experts, dim3((unsigned)groups), dim3(256), MOE_EXPERT_LDS, st, a);
    hipLaunchKernelGGL(k_moe_combine, dim3((unsigned)((rows * 32 + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

}  // namespace eamrl
