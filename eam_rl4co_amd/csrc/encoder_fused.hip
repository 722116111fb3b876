// The whole GraphAttentionNetwork of one instance in ONE workgroup: node embeddings h [M][128] stay in LDS through all
// layers; every Linear runs on v_mfma_f32_16x16x4_f32 with its A operand read from LDS and its B operand (the weights,
// pre-packed on the host into MFMA fragment order) loaded straight from L2 into registers; the self-attention, the
// residuals and the normalisations happen between the GEMM passes without touching HBM.
//
// Reference: rl4co/models/nn/graph/attnnet.py:16-103 (MultiHeadAttentionLayer / GraphAttentionNetwork),
// rl4co/models/nn/attention.py:66-136 (MultiHeadAttention), rl4co/models/nn/ops.py:32-56 (Normalization),
// rl4co/models/nn/mlp.py:52-61 (MLP 128 -> 512 -> 128, ReLU).
//
// Arithmetic = the canonical order of DESIGN.md 2, bit for bit what the unfused kernels of encoder.hip produce:
//   * every Linear output element is chain_k(x[k], W[j][k], K, bias[j]): the f32 MFMA accumulates k in ascending order
//     (k0..k3 inside an instruction, instructions in order), whatever the tile shape;
//   * attention: s = chain_d(q * 0.25, k) (the power-of-two scale folded into q), w = d_expf(s - max),
//     Z = sequential sum of w over the keys (an MFMA against a row of ones: fma(w, 1, Z)), o = chain_j(w, v) / Z;
//   * h = res + y; BatchNorm(eval): fma(h, gamma / sqrt(var + eps), beta - mean * scale); InstanceNorm: sequential sums
//     over the nodes per channel.
//
// LDS layout ("A layout"): element (row, c) of an activation matrix with K columns lives at
//   row * S + (c & 3) * G + (c >> 2)         (G = 34 for K = 128 buffers, 16 for the 64-column head-group buffers)
// so that lane (i = lane & 15, g = lane >> 4) of a 16x16x4 MFMA reads its A values A[i][4t + g], t = 0, 1, ... as
// consecutive floats (ds_read_b64 = two k-steps), and the C layout of a producing MFMA (column = lane & 15,
// row = 4 * (lane >> 4) + reg) stores with plain ds_write_b32.  (S, G) = (140, 34) makes the K = 128 reads bank-conflict
// free and the stores 2-way.
//
// Phases per layer (8 wavefronts: cw = wave & 3 owns a 32-column strip or a head, rw = wave >> 2 a half of the row tiles):
//   for head group hg in {0, 1} (4 heads = 64 columns):
//     P1  q | k | v of the group's heads (wave cw: head 4 hg + cw): q * 0.25 -> QA, k -> KB (A layout), v -> VT (transposed)
//     P2  attention of (head, query tile) units; scores S^T = K Q^T with the keys placed on MFMA rows in the order that
//         makes the accumulators (= softmax weights) the B operand of the value product; o overwrites q in QA
//     P3  out_proj accumulators += att[:, 64 hg .. 64 hg + 63] x Wo^T   (k ascending across the groups)
//   h1 = norm1(h + out_proj) -> HB
//   for chunk c in 0..3 (128 hidden units):  P4 hidden = relu(h1 W1_c^T + b1) -> HID;  P5 ffn2 accumulators += hidden x W2_c^T
//   h2 = norm2(h1 + ffn2) -> HB
#include "encoder_fused.hpp"

namespace eamrl {

constexpr int SA = 140;          // row stride of the K = 128 A-layout buffers (HB, HID)
constexpr int GA = 34;           // their g-stride: (SA, GA) = (140, 34) gives conflict-free ds_read_b64 A fragments AND 2-way (free)
                                 // ds_write_b32 from the C layout; (130, 32) reads as well but stores 4-way (measured: +6 % time)
constexpr int SQ = 66;           // row stride of the 64-column head-group buffers (QA, KB)

// h in the A layout, for the shared stages of encoder_fused.hpp
struct ALayout {
    float* HB;
    static constexpr int S = SA;
    __device__ float* col(int c) const { return HB + (c & 3) * GA + (c >> 2); }
    __device__ void store4(int row, int q4, float4 v) const
    {
        float* p = HB + row * SA + q4;
        p[0] = v.x; p[GA] = v.y; p[2 * GA] = v.z; p[3 * GA] = v.w;
    }
    __device__ float4 load4(int row, int q4) const
    {
        const float* p = HB + row * SA + q4;
        return make_float4(p[0], p[GA], p[2 * GA], p[3 * GA]);
    }
    __device__ void mirror(int, int, float) const {}
};

#ifdef EAMRL_STAMPS   // development build only (tools/build_stamps.sh): per-phase cycle sums over all wavefronts
__device__ unsigned long long g_enc_stamps[24];
#define ESTAMP(i) do { const unsigned long long now_ = __builtin_readcyclecounter(); st_acc[i] += now_ - st_t; st_t = now_; } while (0)
#else
#define ESTAMP(i) do { } while (0)
#endif

// One ds_read_b64.  The A fragments of two k-steps are 8 bytes at an 8-byte-aligned address; read as plain float2 pairs the
// compiler fuses neighbouring ones into ds_read2_b64, which the LDS services in 16-lane groups on 32 banks (8 array cycles,
// and with the (SA, GA) layout 2-way conflicts on top: 16 cycles per pair -- the 46 % conflict cycles of profiles/r02g_pmc_lds_*),
// while two ds_read_b64 take 2 + 2 cycles on 64 banks, conflict-free (MI355X_MICROARCH.md, LDS table).  A volatile access is
// not merged.
typedef float f32x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 lds_read_b64(const float* p)
{
    typedef const volatile __attribute__((address_space(3))) f32x2v* lds_ptr;      // (address-space inference skips volatile accesses)
    const f32x2v v = *(lds_ptr)(p);
    return make_float2(v.x, v.y);
}

// One global_load_dwordx4 of packed weights.  The address space is spelled out: a weight pointer that is carried from one
// phase to the next (the early loads below) is a generic pointer to the compiler, and a flat load counts on the LDS counter
// too, so every wait for an A fragment would also wait for the weights just requested.
__device__ __forceinline__ float4 global_load_b128(const float* p)
{
    typedef const __attribute__((address_space(1))) f32x4* global_ptr;
    const f32x4 v = *(global_ptr)(p);
    return make_float4(v[0], v[1], v[2], v[3]);
}

// First group of B fragments of a pass: issued early (before the previous phase's epilogue / barrier) so that the L2 latency
// of a pass's first weights is not paid behind the barrier.
template <int CT>
__device__ __forceinline__ void load_b0(float4 (&b0)[CT], const float* const (&wp)[CT])
{
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) b0[ct] = global_load_b128(wp[ct]);
}

__device__ __forceinline__ float global_load_b32(const float* p)
{
    typedef const __attribute__((address_space(1))) float* global_ptr;
    return *(global_ptr)(p);
}

// The per-layer constants (CST) are staged in two steps: cst_request issues all loads of a thread's (at most four) entries,
// cst_store folds and writes them to LDS.  Between the two lies whatever hides the latency: the request for layer l + 1 is
// issued ahead of layer l's norm2, the store stays behind the barrier that ends it.
// Thread tid stages the entries tid + 512 t.  Every segment boundary of the CST layout is a multiple of 128, so the segment of
// a trip is uniform over a wave and the pointer is chosen on the wave number wv (an SGPR) with scalar selects -- chosen per
// lane, the compiler fetched the pointer itself with a vector load from the argument block.
//   t = 0: waves 0-5 bqkv, 6-7 bo          t = 1: b1
//   t = 2: waves 0-1 b2, 2-3 norm1 scale, 4-5 norm1 shift, 6-7 norm2 scale          t = 3: waves 0-1 norm2 shift
// so a wave has one normalisation entry, of channel tid & 127, and loads its four operands whatever the kind of norm (instance
// norm may come without running statistics: gamma stands in); b2 is loaded by every wave and stored by waves 0-1.  Nothing
// here sits under a branch.
static_assert(C_BO == 6 * 64 && C_B1 == 512 && C_B2 == 1024 && C_N1 == C_B2 + 2 * 64 && C_N2 == C_N1 + 4 * 64 && NCST == 1536 + 2 * 64,
              "cst_request / cst_store spell out the CST layout");
struct CstRaw { float e0, e1, b2, gamma, beta, mean, var; };

__device__ __forceinline__ CstRaw cst_request(const float* bqkv, const float* bo, const float* b1, const float* b2,
                                              const float* n1_gamma, const float* n1_beta, const float* n1_mean, const float* n1_var,
                                              const float* n2_gamma, const float* n2_beta, const float* n2_mean, const float* n2_var,
                                              int norm, int wv, int tid)
{
    const int c = tid & (FE - 1);
    const bool n1 = wv >= 2 && wv < 6, stats = norm == EAMRL_NORM_BATCH_EVAL;
    const float* gam = n1 ? n1_gamma : n2_gamma;
    const float* mean = n1 ? n1_mean : n2_mean;
    const float* var = n1 ? n1_var : n2_var;
    CstRaw r;
    r.e0 = global_load_b32((wv < 6 ? bqkv : bo) + (tid - (wv < 6 ? 0 : C_BO)));
    r.e1 = global_load_b32(b1 + tid);
    r.b2 = global_load_b32(b2 + c);
    r.gamma = global_load_b32(gam + c);
    r.beta = global_load_b32((n1 ? n1_beta : n2_beta) + c);
    r.mean = global_load_b32((stats ? mean : gam) + c);
    r.var = global_load_b32((stats ? var : gam) + c);
    return r;
}

__device__ __forceinline__ void cst_store(float* CST, const CstRaw r, int norm, float eps, int wv, int tid)
{
    const bool shift = wv < 2 || (wv >= 4 && wv < 6);
    float nv;
    if (norm == EAMRL_NORM_BATCH_EVAL) {
        const float sc = r.gamma / __builtin_sqrtf(r.var + eps);
        const float ms = r.mean * sc;
        nv = shift ? r.beta - ms : sc;
    } else {
        nv = shift ? r.beta : r.gamma;
    }
    CST[tid] = r.e0;
    CST[512 + tid] = r.e1;
    if (wv < 2) {
        CST[1024 + tid] = r.b2;
        CST[1536 + tid] = nv;
    } else {
        CST[1024 + tid] = nv;
    }
}

// First group of A fragments of a pass ([rt][0]: k-steps 0, 1; [rt][1]: k-steps 2, 3).  Where the A buffer is not written by the
// phase before the pass (HB in P1 and P4) they are read ahead of that phase's closing barrier, like the first weights; where
// the barrier publishes the buffer (P3, P5, the Lp pass) right behind it.
template <int RTW, int S>
__device__ __forceinline__ void load_a0(float2 (&a0)[RTW][2], const float* arow, int nrt)
{
#pragma unroll
    for (int rt = 0; rt < RTW; ++rt)
        if (rt < nrt) {
            a0[rt][0] = lds_read_b64(arow + rt * 16 * S);
            a0[rt][1] = lds_read_b64(arow + rt * 16 * S + 2);
        }
}

// acc[rt][ct] += A[rows of tile rt][k] * B[k][cols of tile ct] over NU groups of 4 k-steps (16 k values each).
//   arow: LDS address of this lane's A row of tile 0 (+ g * G), tiles 16 * S floats apart; NU groups start at float offset 0
//   wp[ct]: this lane's float4 of the first group of column tile ct; consecutive groups are 256 floats apart
//   b0, a0: the first group, already loaded (load_b0, load_a0)
// Software pipeline: the A fragments (LDS) and B fragments (L2) of group u + 1 are requested during the MFMAs of group u, into
// a second set of registers.  The compiler's scheduler, left alone, sinks every one of those loads down to its first use (an
// exposed LDS latency every four MFMAs and an exposed L2 latency per group), so the order is pinned: nothing crosses a group
// boundary (sched_barrier), and inside a group the weight loads come first, then one ds_read_b64 behind every second MFMA (a
// block of 2 NRT reads in front of the MFMAs would itself be a bubble), then the remaining MFMAs.
// SWAP: the MFMA takes the weight fragment as A and the activation fragment as B, so that acc[rt][ct] holds the TRANSPOSED
// tile (lane = node row, registers = 4 consecutive output columns): the same products in the same k order, laid out for
// float4 stores to row-major memory.
// NRT: this wave's row tiles as a compile-time value (round 3: as a run-time count every k-step group carried a uniform branch
// around the last tile's loads and MFMAs plus the register copies that merge the two paths)
template <int RTW, int CT, int S, bool SWAP, int NRT, int NU>
__device__ __forceinline__ void gemm_pass_n(f32x4 (&acc)[RTW][CT], const float* arow, const float* const (&wp)[CT],
                                            const float4 (&b0)[CT], const float2 (&a0)[RTW][2])
{
    float4 b[2][CT];
    float2 a[2][NRT][2];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) b[0][ct] = b0[ct];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) { a[0][rt][0] = a0[rt][0]; a[0][rt][1] = a0[rt][1]; }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int c = u & 1, n = c ^ 1;
        __builtin_amdgcn_sched_barrier(0);
        if (u + 1 < NU) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) b[n][ct] = global_load_b128(wp[ct] + (u + 1) * 256);
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
                a[n][rt][0] = lds_read_b64(arow + rt * 16 * S + 4 * (u + 1));
                a[n][rt][1] = lds_read_b64(arow + rt * 16 * S + 4 * (u + 1) + 2);
            }
        }
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
                acc[rt][ct] = SWAP ? mf(b[c][ct].x, a[c][rt][0].x, acc[rt][ct]) : mf(a[c][rt][0].x, b[c][ct].x, acc[rt][ct]);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
                acc[rt][ct] = SWAP ? mf(b[c][ct].y, a[c][rt][0].y, acc[rt][ct]) : mf(a[c][rt][0].y, b[c][ct].y, acc[rt][ct]);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
                acc[rt][ct] = SWAP ? mf(b[c][ct].z, a[c][rt][1].x, acc[rt][ct]) : mf(a[c][rt][1].x, b[c][ct].z, acc[rt][ct]);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
                acc[rt][ct] = SWAP ? mf(b[c][ct].w, a[c][rt][1].y, acc[rt][ct]) : mf(a[c][rt][1].y, b[c][ct].w, acc[rt][ct]);
        }
        if (u + 1 < NU) {       // SchedGroupMask: 0x8 MFMA, 0x20 VMEM read, 0x100 DS read
            __builtin_amdgcn_sched_group_barrier(0x20, CT, 0);
#pragma unroll
            for (int i = 0; i < 2 * NRT; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x8, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x8, 4 * NRT * (CT - 1), 0);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}

// nrt is one of two values per kernel variant: RTW (the first row half) or NLOW (the second)
template <int RTW, int CT, int S, int NU, bool SWAP = false, int NLOW = RTW>
__device__ __forceinline__ void gemm_pass(f32x4 (&acc)[RTW][CT], const float* arow, int nrt, const float* const (&wp)[CT],
                                          const float4 (&b0)[CT], const float2 (&a0)[RTW][2])
{
    if (NLOW == RTW || nrt == RTW) gemm_pass_n<RTW, CT, S, SWAP, RTW, NU>(acc, arow, wp, b0, a0);
    else gemm_pass_n<RTW, CT, S, SWAP, NLOW, NU>(acc, arow, wp, b0, a0);
}

// y = norm(res + acc) for the two column tiles of a wave, written back to HB in place (batch norm: per-column affine;
// instance norm: the sums are written here and normalised per channel after a barrier).
template <int RTW>
__device__ __forceinline__ void residual_norm_store(const f32x4 (&acc)[RTW][2], float* HB, int row0, int nrt, int cw, int j, int G,
                                                    int norm, const float* cst /* LDS: scale [E] | shift [E] */)
{
    asm volatile("" : "+v"(j), "+v"(G));       // addresses rebuilt here, not carried through the layer (see P1's epilogue)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int c = 32 * cw + 16 * ct + j;
        const float sc = cst[c], sh = cst[FE + c];
        float* col = HB + (c & 3) * GA + (c >> 2);
#pragma unroll
        for (int rt = 0; rt < RTW; ++rt)
            if (rt < nrt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float* p = col + (row0 + 16 * rt + 4 * G + r) * SA;
                    float v = *p + acc[rt][ct][r];
                    if (norm == EAMRL_NORM_BATCH_EVAL) v = fma_(v, sc, sh);
                    *p = v;
                }
            }
    }
}

template <int RTT>
__global__ __launch_bounds__(512, 2) void k_encoder_fused(FusedArgs a)
{
    constexpr int RTA = (RTT + 1) / 2;          // row tiles of the first wave half
    constexpr int RTW = RTA;                    // accumulator row tiles per wave
    constexpr int ROWS = 16 * RTT;
    constexpr int SV = ROWS + 4;                // VT row stride
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* HB = lds;                            // [ROWS][SA]   h (residual stream), A layout K = 128
    float* QA = HB + ROWS * SA;                 // [ROWS][SQ]   q * 0.25 of the head group, then the attention output
    float* KB = QA + ROWS * SQ;                 // [ROWS][SQ]   k of the head group
    float* VT = KB + ROWS * SQ;                 // [64][SV]     v of the head group, transposed (column-major)
    float* HID = QA;                            // [ROWS][SA]   FFN hidden chunk (aliases QA | KB | VT, which are dead then)
    float* CST = VT + 64 * SV;                  // [NCST]       the layer's biases and normalisation constants
    static_assert(ROWS * SA <= 2 * ROWS * SQ + 64 * SV, "HID must fit QA | KB | VT");
    const ALayout L{HB};

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform (SGPR): branches on it are scalar branches
    const int cw = wv & 3, rw = wv >> 2;
    const int j = lane & 15, G = lane >> 4;     // C layout: column j, rows 4G + r;  A / B layout: row / column j, k index G
    const int M = a.M;
    const int row0 = rw ? 16 * RTA : 0;         // first row of this wave's tiles
    const int nrt = rw ? RTT - RTA : RTA;       // this wave's row tiles
    const int64_t inst = blockIdx.x;
    const float* hrow = HB + (row0 + j) * SA + G * GA;          // this lane's A row of HB, tile 0
#ifdef EAMRL_STAMPS
    unsigned long long st_acc[22] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, st_t = __builtin_readcyclecounter();
#endif

    // ---- what does not depend on h is requested first, so that one memory latency covers it and the loads of h: layer 0's
    //      constants and the first weights of its P1 (head group 0) ---------------------------------------------------------
    CstRaw cst = cst_request(a.L[0].bqkv, a.L[0].bo, a.L[0].b1, a.L[0].b2, a.L[0].n1_gamma, a.L[0].n1_beta, a.L[0].n1_mean,
                             a.L[0].n1_var, a.L[0].n2_gamma, a.L[0].n2_beta, a.L[0].n2_mean, a.L[0].n2_var, a.norm, wv, tid);
    const float* wp1[3];
    float4 b1[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) wp1[x] = a.L[0].Wqkv + ((int64_t)(8 * x + cw) * (FE / 16)) * 256 + lane * 4;
    load_b0<3>(b1, wp1);
    // ---- h into the A layout; rows >= M are zero ---------------------------------------------------------------------
    if (a.h_in) load_h<ROWS>(a.h_in, M, L);
    else init_embedding<ROWS>(a.init, M, L);
    __syncthreads();
    ESTAMP(0);

    for (int layer = 0; layer < a.nlayers; ++layer) {
        const eamrl_encoder_layer& Ly = a.L[layer];
        // P1 of head group 0: its first weights (wp1, b1) were requested at kernel entry / ahead of the previous layer's norm2,
        // its first A fragments here (h is stable since the barrier that ended the previous layer); those of group 1 ahead of
        // P3 of group 0
        float2 a1[RTW][2];
        load_a0<RTW, SA>(a1, hrow, nrt);
        // ---- the layer's biases and normalisation constants -> LDS (every accumulator is initialised with its bias before
        //      the first MFMA can issue): requested a phase ago (cst_request), so this is a fold and a store, not a load ----
        cst_store(CST, cst, a.norm, a.eps, wv, tid);
        __syncthreads();
        ESTAMP(18);
        // out_proj accumulators: this wave's column tiles 2 cw, 2 cw + 1
        f32x4 acc_o[RTW][2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const float b = CST[C_BO + 32 * cw + 16 * ct + j];
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) acc_o[rt][ct] = splat4(b);
        }
        for (int hg = 0; hg < 2; ++hg) {
            // weights of P3 (this head group's slice of out_proj): first fragments requested now, used after P1 and P2
            const float* wp3[2];
            float4 b3[2];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
                wp3[ct] = Ly.Wo + ((int64_t)(2 * cw + ct) * (FE / 16) + 4 * hg) * 256 + lane * 4;
            // ---- P1: q | k | v of head 4 hg + cw ---------------------------------------------------------------
            {
                f32x4 acc[RTW][3];
                const int ctq = 4 * hg + cw;
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    const float b = CST[C_BQKV + 16 * (8 * x + ctq) + j];
#pragma unroll
                    for (int rt = 0; rt < RTW; ++rt) acc[rt][x] = splat4(b);
                }
                ESTAMP(16);
                gemm_pass<RTW, 3, SA, FE / 16, false, RTT - RTA>(acc, hrow, nrt, wp1, b1, a1);
                ESTAMP(17);
                load_b0<2>(b3, wp3);
                // The lane's coordinates behind an opaque copy: addresses built from j and G are loop invariants, which the
                // compiler otherwise computes once per kernel and carries through P1 -- the phase with the most live registers
                // (RTT = 7: 80 accumulators + two sets of fragments) -- in some 45 VGPRs
                int je = j, Ge = G;
                asm volatile("" : "+v"(je), "+v"(Ge));
                // q (scaled) and k in the A layout of the 64-column buffers: column 16 cw + j -> (g = j & 3, t = 4 cw + (j >> 2))
                float* qcol = QA + (je & 3) * 16 + 4 * cw + (je >> 2);
                float* kcol = KB + (je & 3) * 16 + 4 * cw + (je >> 2);
                float* vrow = VT + (16 * cw + je) * SV;
#pragma unroll
                for (int rt = 0; rt < RTW; ++rt)
                    if (rt < nrt) {
                        const int rbase = row0 + 16 * rt + 4 * Ge;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            qcol[(rbase + r) * SQ] = acc[rt][0][r] * 0.25f;
                            kcol[(rbase + r) * SQ] = acc[rt][1][r];
                        }
                        *reinterpret_cast<float4*>(vrow + rbase) =
                            make_float4(acc[rt][2][0], acc[rt][2][1], acc[rt][2][2], acc[rt][2][3]);
                    }
            }
            ESTAMP(1);
            __syncthreads();
            ESTAMP(2);
            // ---- P2: attention of head cw (of this group), query tiles of this wave half -----------------------------
            {
                int jp = j, Gp = G;            // as in P1's epilogue: P2's addresses are not carried through P1
                asm volatile("" : "+v"(jp), "+v"(Gp));
                // key on MFMA row rho of a key tile: 4 * (rho & 3) + (rho >> 2)  -> accumulator reg r of lane group G holds
                // key 4 r + G, i.e. the B operand of value k-step r
                const int pi = 4 * (jp & 3) + (jp >> 2);
                float kf[RTT][4];
#pragma unroll
                for (int kt = 0; kt < RTT; ++kt) {
                    const float* p = KB + (16 * kt + pi) * SQ + Gp * 16 + 4 * cw;
                    const float2 lo = *reinterpret_cast<const float2*>(p), hi = *reinterpret_cast<const float2*>(p + 2);
                    kf[kt][0] = lo.x; kf[kt][1] = lo.y; kf[kt][2] = hi.x; kf[kt][3] = hi.y;
                }
                float vf[4 * RTT];
                const int NT = (M + 3) >> 2;             // value k-steps (4 keys each)
                constexpr int FULLT = RTT == 7 ? 4 : RTT == 4 ? 2 : 0;       // launch_fused: M > 64 / M > 32 / any
#pragma unroll
                for (int t = 0; t < 4 * RTT; ++t) vf[t] = (t < NT) ? VT[(16 * cw + jp) * SV + 4 * t + Gp] : 0.0f;
                for (int q = 0; q < nrt; ++q) {
                    const int qrow = row0 + 16 * q + jp;
                    const float* qp = QA + qrow * SQ + Gp * 16 + 4 * cw;
                    const float2 qlo = *reinterpret_cast<const float2*>(qp), qhi = *reinterpret_cast<const float2*>(qp + 2);
                    f32x4 s[RTT];
                    float m = -INFINITY;
                    // the four dependent k-steps of a key tile are interleaved with those of the other tiles (an f32 16x16x4
                    // MFMA has a 40-cycle dependent latency against a 32-cycle issue interval)
#pragma unroll
                    for (int kt = 0; kt < RTT; ++kt) s[kt] = mf(kf[kt][0], qlo.x, splat4(0.0f));
#pragma unroll
                    for (int kt = 0; kt < RTT; ++kt) s[kt] = mf(kf[kt][1], qlo.y, s[kt]);
#pragma unroll
                    for (int kt = 0; kt < RTT; ++kt) s[kt] = mf(kf[kt][2], qhi.x, s[kt]);
#pragma unroll
                    for (int kt = 0; kt < RTT; ++kt) s[kt] = mf(kf[kt][3], qhi.y, s[kt]);
#pragma unroll
                    for (int kt = 0; kt < RTT; ++kt) {
                        // (uniform) the tile holds padded keys: the variant's M range leaves the first FULLT tiles always full
                        if (kt >= FULLT && 16 * kt + 16 > M) {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (16 * kt + 4 * r + Gp >= M) s[kt][r] = -INFINITY;
                        }
                        m = vmax5_raw(m, s[kt][0], s[kt][1], s[kt][2], s[kt][3]);      // two v_max3_f32, one asm statement
                    }
                    {   // the four lane groups G share a query: max over lanes l, l^16, l^32, l^48
                        auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
                        m = vmax_raw(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
                        auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
                        m = vmax_raw(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
                    }
#pragma unroll
                    for (int kt = 0; kt < RTT; ++kt) {      // packed fp32 math, the two pairs of a tile statement by statement: each
                        f32x2 e01 = (f32x2){s[kt][0], s[kt][1]} - splat2(m), e23 = (f32x2){s[kt][2], s[kt][3]} - splat2(m);
                        d_expf2_nonpos_x2(e01, e23);                                          // element bit-identical to d_expf
                        s[kt] = (f32x4){e01.x, e01.y, e23.x, e23.y};
                    }
                    // Z (canonical order, encoder.hip ZRot): this lane holds the keys 4 r + G of every tile, i.e. one residue class
                    // mod 4 in ascending order -> its partial sum P_G in 4 RTT - 1 adds, then (P0 + P1) + (P2 + P3) over the lane groups
                    float zp = s[0][0];
#pragma unroll
                    for (int t = 1; t < 4 * RTT; ++t) zp = zp + s[t >> 2][t & 3];
                    {
                        auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(zp), __float_as_uint(zp), false, false);
                        zp = __uint_as_float(r16[0]) + __uint_as_float(r16[1]);
                        auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(zp), __float_as_uint(zp), false, false);
                        zp = __uint_as_float(r32[0]) + __uint_as_float(r32[1]);
                    }
                    f32x4 o = splat4(0.0f);
#pragma unroll
                    for (int kt = 0; kt < RTT; ++kt)        // a (uniform) test per key tile that may be empty, none per k-step: the padded
                                                            // k-steps of a started tile multiply zero weights with zero values, and
                                                            // fma(0, 0, o) == o (o is never -0: it starts from +0)
                        if (kt < FULLT || 16 * kt < M) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) o = mf(vf[4 * kt + r], s[kt][r], o);
                        }
                    // o: lane (query j, G), reg r -> head column e = 4 G + r -> A layout (g = r, t = 4 cw + G); overwrites q
                    float* op = QA + qrow * SQ + 4 * cw + Gp;
#pragma unroll
                    for (int r = 0; r < 4; ++r) op[r * 16] = o[r] / zp;
                }
            }
            ESTAMP(3);
            __syncthreads();
            ESTAMP(4);
            // ---- P3: out_proj partial over the 64 attention columns of this head group ------------------------------
            float2 a3[RTW][2];
            load_a0<RTW, SQ>(a3, QA + (row0 + j) * SQ + G * 16, nrt);
            if (hg == 0) {                     // P1 of head group 1 starts behind P3's barrier, which leaves h alone
#pragma unroll
                for (int x = 0; x < 3; ++x) wp1[x] += 4 * (FE / 16) * 256;
                load_b0<3>(b1, wp1);
                load_a0<RTW, SA>(a1, hrow, nrt);
            }
            gemm_pass<RTW, 2, SQ, 4, false, RTT - RTA>(acc_o, QA + (row0 + j) * SQ + G * 16, nrt, wp3, b3, a3);
            ESTAMP(5);
            __syncthreads();
            ESTAMP(6);
        }
        // P4 of chunk 0: first weights now; its first A fragments are h1, which the barrier below publishes
        const float* wp4[2];
        float4 b4[2];
        float2 a4[RTW][2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) wp4[ct] = Ly.W1 + ((int64_t)(2 * cw + ct) * (FE / 16)) * 256 + lane * 4;
        load_b0<2>(b4, wp4);
        // ---- h1 = norm1(h + out_proj) -> HB ----------------------------------------------------------------------------
        residual_norm_store<RTW>(acc_o, HB, row0, nrt, cw, j, G, a.norm, CST + C_N1);
        __syncthreads();
        if (a.norm == EAMRL_NORM_INSTANCE) {
            instance_norm(L, M, a.eps, CST + C_N1);
            __syncthreads();
        }
        load_a0<RTW, SA>(a4, hrow, nrt);
        ESTAMP(7);
        // ---- FFN: 4 chunks of 128 hidden units ---------------------------------------------------------------------------
        f32x4 acc_f[RTW][2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const float b = CST[C_B2 + 32 * cw + 16 * ct + j];
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) acc_f[rt][ct] = splat4(b);
        }
        for (int ch = 0; ch < FF / 128; ++ch) {
            const float* wp5[2];
            float4 b5[2];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
                wp5[ct] = Ly.W2 + ((int64_t)(2 * cw + ct) * (FF / 16) + 8 * ch) * 256 + lane * 4;
            {   // P4: hidden chunk = relu(h1 W1_ch^T + b1) -> HID
                f32x4 acc[RTW][2];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const float b = CST[C_B1 + 16 * (8 * ch + 2 * cw + ct) + j];
#pragma unroll
                    for (int rt = 0; rt < RTW; ++rt) acc[rt][ct] = splat4(b);
                }
                ESTAMP(14);
                gemm_pass<RTW, 2, SA, FE / 16, false, RTT - RTA>(acc, hrow, nrt, wp4, b4, a4);
                ESTAMP(15);
                load_b0<2>(b5, wp5);           // P5's first weights fly during the epilogue and the barrier
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const int c = 32 * cw + 16 * ct + j;
                    float* col = HID + (c & 3) * GA + (c >> 2);
#pragma unroll
                    for (int rt = 0; rt < RTW; ++rt)
                        if (rt < nrt) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float v = acc[rt][ct][r];
                                col[(row0 + 16 * rt + 4 * G + r) * SA] = !(v > 0.0f) ? 0.0f : v;
                            }
                        }
                }
            }
            ESTAMP(8);
            __syncthreads();
            ESTAMP(9);
            // P5: ffn2 accumulators += hidden chunk x W2[:, 128 ch .. 128 ch + 127]^T
            float2 a5[RTW][2];
            load_a0<RTW, SA>(a5, HID + (row0 + j) * SA + G * GA, nrt);
            if (ch + 1 < FF / 128) {           // P4 of the next chunk starts behind P5's barrier, which leaves h1 alone
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) wp4[ct] += 8 * (FE / 16) * 256;
                load_b0<2>(b4, wp4);
                load_a0<RTW, SA>(a4, hrow, nrt);
            }
            gemm_pass<RTW, 2, SA, 8, false, RTT - RTA>(acc_f, HID + (row0 + j) * SA + G * GA, nrt, wp5, b5, a5);
            ESTAMP(10);
            __syncthreads();
            ESTAMP(11);
        }
        // ---- the next layer's constants and P1 weights fly during norm2 (after the last layer: the same layer again, unused) ----
        {
            const eamrl_encoder_layer& Ln = a.L[layer + 1 < a.nlayers ? layer + 1 : layer];
            cst = cst_request(Ln.bqkv, Ln.bo, Ln.b1, Ln.b2, Ln.n1_gamma, Ln.n1_beta, Ln.n1_mean, Ln.n1_var, Ln.n2_gamma, Ln.n2_beta,
                              Ln.n2_mean, Ln.n2_var, a.norm, wv, tid);
#pragma unroll
            for (int x = 0; x < 3; ++x) wp1[x] = Ln.Wqkv + ((int64_t)(8 * x + cw) * (FE / 16)) * 256 + lane * 4;
            load_b0<3>(b1, wp1);
        }
        // ---- h2 = norm2(h1 + ffn) -> HB ------------------------------------------------------------------------------------
        residual_norm_store<RTW>(acc_f, HB, row0, nrt, cw, j, G, a.norm, CST + C_N2);
        __syncthreads();
        if (a.norm == EAMRL_NORM_INSTANCE) {
            instance_norm(L, M, a.eps, CST + C_N2);
            __syncthreads();
        }
        ESTAMP(12);
    }
    // ---- store h; skipped when the caller keeps only the decoder cache ----------------------------------------------------
    if (a.h_out) store_h(a.h_out, M, L);
    ESTAMP(13);
    // the first weights of cache pass 0 fly during the graph context; those of pass sl + 1 during the global stores of pass sl
    // (no branch around the request -- a load under a branch makes the graph context wait for it; without a cache it reads
    // layer 0's weights, unused)
    const float* wpc[2];
    float4 bc[2];
    {
        const float* w0 = !a.cache.out ? a.L[0].Wqkv : a.cache.nproj == 0 ? a.cache.WoutT : a.cache.Wc;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) wpc[ct] = w0 + ((int64_t)(2 * cw + ct) * (FE / 16)) * 256 + lane * 4;
        load_b0<2>(bc, wpc);
    }
    if (a.cache.gctx) graph_context(a.cache.Wg, a.cache.gctx, M, L, CST);          // the layer constants are dead
    ESTAMP(19);
    // ---- decoder cache from the resident embeddings: nproj projections of h, then Lp = L Wout ------------------------------
    if (a.cache.out) {
        float* STG = QA;                           // L in the A layout (operand of the Lp pass); aliases the dead attention buffers
        float* crow = a.cache.out + (inst * (int64_t)M) * a.cache.ld;
        for (int sl = 0; sl <= a.cache.nproj; ++sl) {
            const bool lp = sl == a.cache.nproj;
            f32x4 acc[RTW][2];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int rt = 0; rt < RTW; ++rt) acc[rt][ct] = splat4(0.0f);
            if (lp) __syncthreads();               // every wave's part of L is in STG
            const float* arow = (lp ? STG : HB) + (row0 + j) * SA + G * GA;
            float2 a0[RTW][2];
            load_a0<RTW, SA>(a0, arow, nrt);
            gemm_pass<RTW, 2, SA, FE / 16, true, RTT - RTA>(acc, arow, nrt, wpc, bc, a0);
            {   // the next pass (after the last one: the same weights again, unused; no branch around a load)
                const int sn = lp ? sl : sl + 1;
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
                    wpc[ct] = (sn == a.cache.nproj ? a.cache.WoutT : a.cache.Wc + (int64_t)sn * FE * FE) +
                              ((int64_t)(2 * cw + ct) * (FE / 16)) * 256 + lane * 4;
                load_b0<2>(bc, wpc);
            }
            // transposed tiles: lane = node row0 + 16 rt + j, registers = output columns 32 cw + 16 ct + 4 G + (0..3)
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
                        if (sl == 2) {             // L also feeds the Lp pass: element (node, c + r) -> A layout (g = r, t = c / 4)
                            float* p = STG + node * SA + (c >> 2);
                            p[0] = v[0]; p[GA] = v[1]; p[2 * GA] = v[2]; p[3 * GA] = v[3];
                        }
                    }
                }
        }
    }
    ESTAMP(21);
#ifdef EAMRL_STAMPS
    if (lane == 0) {       // [20] counts the wavefronts; [18] constants staging, [19] graph context, [21] cache passes
        for (int i = 0; i < 22; ++i)
            if (i != 20) atomicAdd(&g_enc_stamps[i], st_acc[i]);
        atomicAdd(&g_enc_stamps[20], 1ull);
    }
#endif
}

// Wp[ct][u][16 g + j][q] = W[16 ct + j][16 u + 4 q + g]: lane (j, g) of a 16x16x4 MFMA finds its B values of four consecutive
// k-steps in one float4, and a wavefront's 64 float4 are 1 KB contiguous.
__global__ void k_pack_mfma_b(const float* __restrict__ W, float* __restrict__ Wp, int N, int K)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)N * K) return;
    const int q = (int)(idx & 3), l = (int)((idx >> 2) & 63);
    const int64_t blk = idx >> 8;                 // ct * (K / 16) + u
    const int u = (int)(blk % (K / 16)), ct = (int)(blk / (K / 16));
    const int j = l & 15, g = l >> 4;
    Wp[idx] = W[(int64_t)(16 * ct + j) * K + 16 * u + 4 * q + g];
}

int launch_pack_mfma_b(const float* W, float* Wp, int N, int K, hipStream_t st)
{
    const int64_t n = (int64_t)N * K;
    hipLaunchKernelGGL(k_pack_mfma_b, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, W, Wp, N, K);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

#ifdef EAMRL_STAMPS
extern "C" __attribute__((visibility("default"))) int eamrl_debug_read_enc_stamps(unsigned long long* out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_enc_stamps), sizeof(g_enc_stamps)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[24] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_enc_stamps), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

bool encoder_fused_supports(int M, int E, int H, int FFdim, int nlayers)
{
    return M >= 1 && M <= 112 && E == FE && H == FH && FFdim == FF && nlayers >= 1 && nlayers <= MAX_FUSED_LAYERS;
}

int launch_encoder_fused(const float* h_in, float* h_out, int64_t B, int M, int nlayers, int norm, float eps,
                         const eamrl_encoder_layer* layers, const eamrl_encoder_cache* cache, const eamrl_encoder_init* init,
                         int dtype, hipStream_t st)
{
    if (B <= 0) return 0;
    FusedArgs a = {};
    a.h_in = init ? nullptr : h_in; a.h_out = h_out; a.M = M; a.nlayers = nlayers; a.norm = norm; a.eps = eps;
    if (cache) {
        a.cache = *cache;
        if (!cache->Wg || !cache->gctx) a.cache.Wg = a.cache.gctx = nullptr;
    }
    if (init) a.init = *init;
    for (int l = 0; l < nlayers; ++l) a.L[l] = layers[l];
    if (dtype != DTYPE_F32) return launch_encoder_fused16(a, B, dtype, st);
    return launch_fused(a, B, st, [](auto rtt) {
        constexpr int RTT = decltype(rtt)::value, ROWS = 16 * RTT;
        return FusedVariant{k_encoder_fused<RTT>, ((size_t)ROWS * SA + 2 * (size_t)ROWS * SQ + 64 * (size_t)(ROWS + 4) + NCST) * sizeof(float)};
    });
}

}  // namespace eamrl
