// EAS-Lay backward on fp32 MFMA: the gradient of the per-instance residual layer that k_rollout_ms_mfma<..., LayArgs> applies
// between the glimpse and the logits (eamrl_eas_layer_backward).
//
// Reference: rl4co/models/zoo/eas/nn.py:5-30 (the layer), zoo/eas/decoder.py:12-32 (its place: on the heads, before
// project_out) and the autograd step of zoo/eas/search.py:202-259.  For obj = sum glogp[r,t] logp[r,t] and every decode step
//     pre = h W1[b] + b1[b];  a = relu(pre);  y = h + a W2[b] + b2[b];  u[n] = y . Lp[b][n];  z = process(u / sqrt(E));  logp = z[act] - lse
//     dY = du Lp[b];  dW2[b] += a^T dY;  db2[b] += sum dY;  dpre = (dY W2[b]^T) o [pre > 0];  dW1[b] += h^T dpre;  db1[b] += sum dpre
// The logits of y, du (the normaliser recovered from the rollout's log-prob when no lse is given) and dY are the stages of
// reeval_tile.hpp that the re-evaluation backward kernels of reeval.hip run: logit_tile on the y tile, logit_bwd_tile,
// lpt_du.  A step with one feasible node and a step past heads_T take no gradient: that is this kernel's own `live`, which enters
// logit_bwd_tile as g = 0.  h is the rollout's captured glimpse output (eamrl_reeval.heads): nothing upstream of it is adapted,
// so there is no dh, no glimpse backward and no gather.
//
// Structure: the grid and 16-query tiling of k_reeval_bwd_lp -- one workgroup of 8 wavefronts per (instance, row chunk).  Wave w
// owns the columns 16 w .. 16 w + 15 of pre / a / y / dY / dpre and the rows 16 w .. 16 w + 15 of dW1 and dW2: 2 x 8 accumulator
// tiles = 64 registers per lane, kept across all tiles and flushed once with float atomics (nchunk workgroups share an
// instance).  The forward weights stream from L2 in fragment order (w_load / w_gemm of mfma_tile.hpp, as in the rollout kernel);
// the wave's 16 rows of W2 for the dpre product (contraction over W2's columns) are 32 registers, loaded once.  Tiles are not
// software-pipelined: seven barriers per tile (eight when the normaliser is recovered).  LDS: LayLds.
#include "reeval_tile.hpp"

namespace eamrl {

namespace {

template <int RTT>
struct LayLds {         // the kernel's dynamic LDS (float offsets): its carve-up and the byte count at its launch both read this
    static constexpr int HT = 0;                        // [16][TS]  h
    static constexpr int AT = HT + 16 * TS;             // [16][TS]  a = relu(pre)
    static constexpr int YT = AT + 16 * TS;             // [16][TS]  y, then dpre
    static constexpr int DYT = YT + 16 * TS;            // [16][TS]  dY
    static constexpr int DU = DYT + 16 * TS;            // [16 RTT][DS]
    static constexpr int LSE = DU + 16 * RTT * DS;      // [16]
    static constexpr int LPT = LSE + 16;                // [8 waves][RTT][64 lanes][4]  Lp^T fragments of the dY product
    static constexpr int END = LPT + 8 * RTT * 256;
    static constexpr size_t bytes = (size_t)END * sizeof(float);
};

template <int RTT>
__global__ __launch_bounds__(512) void k_eas_layer_bwd(ReevalArgs a, eamrl_eas_layer ly)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using L = LayLds<RTT>;
    float *HT = lds + L::HT, *AT = lds + L::AT, *YT = lds + L::YT, *DYT = lds + L::DYT, *DU = lds + L::DU, *LSE = lds + L::LSE;
    float* LPT = lds + L::LPT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, G = lane >> 4;
    const int jq = tid >> 5, e4 = tid & 31;
    const int64_t b = blockIdx.x / a.nchunk;
    const int ch = (int)(blockIdx.x - b * a.nchunk);
    const int s0 = (int)((int64_t)a.S * ch / a.nchunk), s1 = (int)((int64_t)a.S * (ch + 1) / a.nchunk);
    const int ns = s1 - s0, T = a.T;
    const int ntiles = (ns * T + 15) / 16;
    const bool derive_lse = a.lse == nullptr;       // logp = the rollout's log-probs: the normaliser is z[action] - logp
    const float inv_temp = 1.0f / a.temp;
    const float* W1b = ly.W1 + b * (RE * RE);
    const float* W2b = ly.W2 + b * (RE * RE);

    // ---- instance operands (once) --------------------------------------------------------------------------------------
    float lpf[32];                                  // Lp rows of key tile wv (keys in pi order)
    load_lp_frags(a, b, wv < RTT ? wv : RTT - 1, lane, lpf);       // (waves >= RTT compute no logits)
    float4* lpt = reinterpret_cast<float4*>(LPT) + wv * RTT * 64 + lane;
    fill_lpt<RTT>(a, b, wv, lane, lpt);
    // W2 rows 16 wv + j as the A operand of dpre = dY W2^T: w2r[t] = W2[16 wv + j][4 t + G], picked out of the fragment order
    // (block float 4 ((T 8 + q) 64 + l) + i holds W[16 q + 4 i + l / 16][16 T + l % 16])
    float w2r[32];
#pragma unroll
    for (int t = 0; t < 32; ++t)
        w2r[t] = W2b[4 * (((t >> 2) * 8 + wv) * 64 + 16 * (j & 3) + 4 * (t & 3) + G) + (j >> 2)];
    const float4 bb1 = *reinterpret_cast<const float4*>(ly.b1 + b * RE + 16 * wv + 4 * G);
    const float4 bb2 = *reinterpret_cast<const float4*>(ly.b2 + b * RE + 16 * wv + 4 * G);
    f32x4 dW1[8], dW2[8], db1a = z4(), db2a = z4();
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) { dW1[nt] = z4(); dW2[nt] = z4(); }

    auto qi_of = [&](const QWalk& w) -> int { return w.sl < ns ? ((s0 + w.sl) * (int)a.B + (int)b) * T + w.t : -1; };
    QWalk wr, wj;                       // the staging role (query jq) and the MFMA role (query j) of this thread
    wr.init(jq, T);
    wj.init(j, T);

    for (int tile = 0; tile < ntiles; ++tile) {
        // ---- stage h: thread (query jq, columns 4 e4 ..); zeros for a query that does not exist or takes no gradient --------
        {
            const int qi = qi_of(wr);
            const int th = wr.t - a.tstart;
            float4 hv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (qi >= 0 && th >= 0 && th < a.heads_T) {
                const int64_t r = (int64_t)(s0 + wr.sl) * a.B + b;
                hv = *reinterpret_cast<const float4*>(a.heads + (r * a.heads_T + th) * RE + 4 * e4);
            }
            float* dp = HT + jq * TS + e4;
            dp[0] = hv.x; dp[TG] = hv.y; dp[2 * TG] = hv.z; dp[3 * TG] = hv.w;
            wr.next(T);
        }
        // ---- this lane's query (MFMA role) ---------------------------------------------------------------------------------
        const int qj = qi_of(wj), tj = wj.t;
        wj.next(T);
        const int qjc = max(qj, 0);
        uint4 mb = make_uint4(0, 0, 0, 0);
        if (qj >= 0) mb = *reinterpret_cast<const uint4*>(a.maskbits + (int64_t)qjc * 4);
        const int nfeas = __popc(mb.x) + __popc(mb.y) + __popc(mb.z) + __popc(mb.w);
        // (a step with one feasible node has p = 1 and takes no gradient: an exact zero, whatever the rounding of exp)
        const bool live = qj >= 0 && tj >= a.tstart && tj - a.tstart < a.heads_T && nfeas > 1;
        const int act = qj >= 0 ? (int)a.actions[qjc] : -1;
        const float g = live ? a.glogp[qjc] : 0.0f;
        const float lse = live ? (derive_lse ? a.logp[qjc] : a.lse[qjc]) : 0.0f;
        f32x4 wa[PQ], wb[PQ];
        w_load(wa, W1b, 2 * wv, lane);
        w_load(wb, W1b, 2 * wv + 1, lane);
        __syncthreads();                // (1) h is published
        // ---- pre = h W1 + b1, a = relu(pre): lane (query j, G), register r <-> column 16 wv + 4 G + r -------------------------
        f32x4 hown;
        uint32_t pos = 0;
        {
            const float* hp = HT + j * TS + G * TG;
            const float* ho = HT + j * TS + 4 * wv + G;
#pragma unroll
            for (int r = 0; r < 4; ++r) hown[r] = ho[r * TG];
            f32x4 p0 = (f32x4){bb1.x, bb1.y, bb1.z, bb1.w}, p1 = z4();
            w_gemm(wa, hp, p0, p1);
            w_load(wa, W2b, 2 * wv, lane);
            w_gemm(wb, hp + 16, p0, p1);
            w_load(wb, W2b, 2 * wv + 1, lane);
            const f32x4 pr = p0 + p1;
            float* ap = AT + j * TS + 4 * wv + G;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (pr[r] > 0.0f) pos |= 1u << r;
                ap[r * TG] = pr[r] > 0.0f ? pr[r] : 0.0f;
            }
        }
        __syncthreads();                // (2) a is published
        // ---- y = h + a W2 + b2 ------------------------------------------------------------------------------------------------
        {
            const float* ap = AT + j * TS + G * TG;
            f32x4 q0 = (f32x4){bb2.x, bb2.y, bb2.z, bb2.w}, q1 = z4();
            w_gemm(wa, ap, q0, q1);
            w_gemm(wb, ap + 16, q0, q1);
            const f32x4 y = hown + (q0 + q1);
            float* yp = YT + j * TS + 4 * wv + G;
#pragma unroll
            for (int r = 0; r < 4; ++r) yp[r * TG] = y[r];
        }
        __syncthreads();                // (3) y is published
        // ---- logits of key tile wv (of y) and du; the eighth barrier is inside, when the normaliser is recovered -----------------
        {
            f32x4 u = z4();
            if (wv < RTT) u = logit_tile(lpf, YT, lane);
            logit_bwd_tile(u, wv < RTT, wv, lane, mb, act, g, lse, derive_lse, a.clip, inv_temp, LSE, DU);
        }
        __syncthreads();                // (4) du is published
        // ---- dY = du Lp: columns 16 wv + 4 G + r of query j -------------------------------------------------------------------
        {
            const f32x4 dy = lpt_du<RTT>(lpt, DU, lane);
            float* yp = DYT + j * TS + 4 * wv + G;
#pragma unroll
            for (int r = 0; r < 4; ++r) yp[r * TG] = dy[r];
            db2a = db2a + dy;
        }
        __syncthreads();                // (5) dY is published; every wave has read y
        // ---- dpre = (dY W2^T) o [pre > 0]: rows 16 wv + 4 G + r of W2, query j -------------------------------------------------
        {
            const float* yp = DYT + j * TS + G * TG;
            f32x4 d0 = z4(), d1 = z4();
#pragma unroll
            for (int t = 0; t < 32; t += 2) {
                d0 = mf(w2r[t], yp[t], d0);
                d1 = mf(w2r[t + 1], yp[t + 1], d1);
            }
            f32x4 dp = d0 + d1;
            float* pp = YT + j * TS + 4 * wv + G;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dp[r] = ((pos >> r) & 1u) ? dp[r] : 0.0f;
                pp[r * TG] = dp[r];
            }
            db1a = db1a + dp;
        }
        __syncthreads();                // (6) dpre is published
        // ---- dW2 += a^T dY, dW1 += h^T dpre: wave wv the rows 16 wv .. + 15, contraction over the tile's 16 queries --------------
        {
            float aa[4], ha[4];
            load_tile_col(AT, wv, lane, aa);
            load_tile_col(HT, wv, lane, ha);
#pragma unroll
            for (int nt = 0; nt < 8; ++nt) {
                const int c2 = 16 * nt + j;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int o = (4 * t + G) * TS + a_off(c2);
                    dW2[nt] = mf(aa[t], DYT[o], dW2[nt]);
                    dW1[nt] = mf(ha[t], YT[o], dW1[nt]);
                }
            }
        }
        __syncthreads();                // (7) the tiles are free for the next round
    }
    // ---- flush: lane (column n = 16 nt + j, G), register r -> row k = 16 wv + 4 G + r, in the parameters' fragment order -------
    float* gW1 = ly.dW1 + b * (RE * RE);
    float* gW2 = ly.dW2 + b * (RE * RE);
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = 4 * ((nt * 8 + wv) * 64 + 16 * r + j) + G;
            atomicAdd(gW1 + o, dW1[nt][r]);
            atomicAdd(gW2 + o, dW2[nt][r]);
        }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float s1v = row16_sum(db1a[r]), s2v = row16_sum(db2a[r]);
        if (j == 0) {
            atomicAdd(ly.db1 + b * RE + 16 * wv + 4 * G + r, s1v);
            atomicAdd(ly.db2 + b * RE + 16 * wv + 4 * G + r, s2v);
        }
    }
}

template <int RTT>
int launch_t(const ReevalArgs& a, const eamrl_eas_layer& ly, hipStream_t st)
{
    const size_t lds = LayLds<RTT>::bytes;
    static_assert(lds == (size_t)(4 * 16 * TS + 16 * RTT * DS + 16 + 8 * RTT * 256) * sizeof(float), "the byte count spelled out before LayLds");
    auto k = k_eas_layer_bwd<RTT>;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return EAMRL_E_LAUNCH;
    hipLaunchKernelGGL(k, dim3((unsigned)(a.B * a.nchunk)), dim3(512), lds, st, a, ly);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

}  // namespace

int launch_eas_layer_bwd(const ReevalArgs& a, const eamrl_eas_layer& ly, hipStream_t st)
{
    if (a.M <= 32) return launch_t<2>(a, ly, st);
    if (a.M <= 64) return launch_t<4>(a, ly, st);
    return launch_t<7>(a, ly, st);
}

}  // namespace eamrl
