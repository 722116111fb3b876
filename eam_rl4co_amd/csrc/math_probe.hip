// Test support: runs the functions of dmath.hpp one by one, so that tests/test_gpu_math.py can hold each of them to the oracle
// bit for bit.  Compiled with the library's own flags (-ffp-contract=off, IEEE divide), so the functions are built here exactly
// as in the kernels that include the header.  The probes CALL the header's functions; nothing of them is restated here, and no
// product path calls a probe.  (What is pinned is the header's function, not each inlined copy in the including files.)
#include "dmath.hpp"

#include "../../include/eamrl.h"

namespace eamrl {

// ---- elementwise probe: one thread = four consecutive elements = the 4 / 2+2 / 1+1+1+1 slots of the wide forms ----------------
template <int FN>
__global__ void k_math_probe(const uint32_t* __restrict__ x, uint32_t* __restrict__ y, int64_t n)
{
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (i0 >= n) return;                       // n is a multiple of 4 (checked by the entry point)
    if constexpr (FN == EAMRL_PROBE_PHILOX) {  // case = i0 / 4: six input words (counter, key) -> four output words
        const uint32_t* c = x + 6 * (i0 >> 2);
        const u32x4 r = philox4x32_10(c[0], c[1], c[2], c[3], c[4], c[5]);
        y[i0] = r.x; y[i0 + 1] = r.y; y[i0 + 2] = r.z; y[i0 + 3] = r.w;
        return;
    } else if constexpr (FN == EAMRL_PROBE_EXP1_FROM_BITS) {
#pragma unroll
        for (int k = 0; k < 4; ++k) y[i0 + k] = __float_as_uint(exp1_from_bits(x[i0 + k]));
        return;
    } else {
        float a[4], o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = __uint_as_float(x[i0 + k]);
        if constexpr (FN == EAMRL_PROBE_EXPF || FN == EAMRL_PROBE_LOGF || FN == EAMRL_PROBE_RCPF || FN == EAMRL_PROBE_TANHF) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                o[k] = FN == EAMRL_PROBE_EXPF ? d_expf(a[k]) : FN == EAMRL_PROBE_LOGF ? d_logf(a[k]) : FN == EAMRL_PROBE_RCPF ? d_rcpf(a[k]) : d_tanhf(a[k]);
        } else if constexpr (FN == EAMRL_PROBE_EXPF2 || FN == EAMRL_PROBE_EXPF2_NONPOS || FN == EAMRL_PROBE_TANHF2) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x2 v = {a[2 * h], a[2 * h + 1]};
                const f32x2 r = FN == EAMRL_PROBE_EXPF2 ? d_expf2(v) : FN == EAMRL_PROBE_EXPF2_NONPOS ? d_expf2_nonpos(v) : d_tanhf2(v);
                o[2 * h] = r.x; o[2 * h + 1] = r.y;
            }
        } else if constexpr (FN == EAMRL_PROBE_EXPF2_NONPOS_X2) {
            f32x2 p = {a[0], a[1]}, q = {a[2], a[3]};
            d_expf2_nonpos_x2(p, q);
            o[0] = p.x; o[1] = p.y; o[2] = q.x; o[3] = q.y;
        } else {
            const f32x4m v = {a[0], a[1], a[2], a[3]};
            const f32x4m r = FN == EAMRL_PROBE_EXPF4 ? d_expf4(v) : FN == EAMRL_PROBE_EXPF4_NONPOS ? d_expf4_nonpos(v) : FN == EAMRL_PROBE_LOGF4 ? d_logf4(v) : d_tanhf4(v);
            o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) y[i0 + k] = __float_as_uint(o[k]);
    }
}

// ---- wavefront probe: one 64-lane workgroup = one wavefront = one case; every lane is live (the DPP forms assume a full exec
// mask) and every lane stores what it ends with ---------------------------------------------------------------------------------
template <int FN>
__global__ __launch_bounds__(EAMRL_WAVE) void k_wave_probe(const uint32_t* __restrict__ v, const int32_t* __restrict__ idx,
                                                           uint32_t* __restrict__ out_v, int32_t* __restrict__ out_i)
{
    const int l = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * EAMRL_WAVE;
    const uint32_t* row = v + base;
    auto at = [&](int k) { return __uint_as_float(row[(l + k) & (EAMRL_WAVE - 1)]); };   // lane-local operand k: the value k lanes on
    float r;
    if constexpr (FN == EAMRL_WPROBE_TREE_SUM) {
        r = wave_tree_sum(at(0));
    } else if constexpr (FN == EAMRL_WPROBE_MAX) {
        r = wave_max(at(0));
    } else if constexpr (FN == EAMRL_WPROBE_ARGMAX) {
        r = at(0);
        int i = idx[base + l];
        wave_argmax(r, i);
        out_i[base + l] = i;
    } else if constexpr (FN == EAMRL_WPROBE_VMAX) {
        r = vmax_raw(at(0), at(1));
    } else if constexpr (FN == EAMRL_WPROBE_VMAX3) {
        r = vmax3_raw(at(0), at(1), at(2));
    } else if constexpr (FN == EAMRL_WPROBE_VMAX5) {
        r = vmax5_raw(at(0), at(1), at(2), at(3), at(4));
    } else {
        // nodes start .. n1 - 1, node n of lane l weighs v[(l + n - start) % 64]; the run length is clamped so that a bad idx
        // cannot stall the wavefront (reads stay inside the row whatever it is)
        const int start = idx[base], n1 = idx[base + 1];
        int len = n1 - start;
        len = len < 0 ? 0 : (len > 1024 ? 1024 : len);
        if constexpr (FN == EAMRL_WPROBE_ZROT) {
            ZRot<float> z{0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < len; ++k) z.add(at(k));
            r = z.total(n1);
        } else {
            float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int k0 = 0; k0 < len; k0 += 4) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k0 + j < len) z[j] = z[j] + at(k0 + j);
            }
            r = z_total_rel(z[0], z[1], z[2], z[3], start);
        }
    }
    out_v[base + l] = __float_as_uint(r);
}

template <int FN>
static int launch_math(const uint32_t* x, uint32_t* y, int64_t n, hipStream_t st)
{
    const int64_t groups = n / 4;
    hipLaunchKernelGGL(k_math_probe<FN>, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, x, y, n);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

template <int FN>
static int launch_wave(const uint32_t* v, const int32_t* idx, uint32_t* out_v, int32_t* out_i, int64_t nwaves, hipStream_t st)
{
    hipLaunchKernelGGL(k_wave_probe<FN>, dim3((unsigned)nwaves), dim3(EAMRL_WAVE), 0, st, v, idx, out_v, out_i);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

}  // namespace eamrl

using namespace eamrl;

extern "C" {

__attribute__((visibility("default"))) int eamrl_math_probe(int fn, const uint32_t* x, uint32_t* y, int64_t n, void* stream)
{
    if (!x || !y || n < 0 || (n & 3) || n > ((int64_t)1 << 32)) return EAMRL_E_ARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    switch (fn) {
#define EAMRL_CASE(F) case F: return launch_math<F>(x, y, n, st)
        EAMRL_CASE(EAMRL_PROBE_EXPF); EAMRL_CASE(EAMRL_PROBE_EXPF2); EAMRL_CASE(EAMRL_PROBE_EXPF2_NONPOS);
        EAMRL_CASE(EAMRL_PROBE_EXPF2_NONPOS_X2); EAMRL_CASE(EAMRL_PROBE_EXPF4); EAMRL_CASE(EAMRL_PROBE_EXPF4_NONPOS);
        EAMRL_CASE(EAMRL_PROBE_LOGF); EAMRL_CASE(EAMRL_PROBE_LOGF4); EAMRL_CASE(EAMRL_PROBE_RCPF); EAMRL_CASE(EAMRL_PROBE_TANHF);
        EAMRL_CASE(EAMRL_PROBE_TANHF2); EAMRL_CASE(EAMRL_PROBE_TANHF4); EAMRL_CASE(EAMRL_PROBE_EXP1_FROM_BITS);
        EAMRL_CASE(EAMRL_PROBE_PHILOX);
#undef EAMRL_CASE
    }
    return EAMRL_E_ARG;
}

__attribute__((visibility("default"))) int eamrl_wave_probe(int fn, const uint32_t* v, const int32_t* idx, uint32_t* out_v,
                                                           int32_t* out_i, int64_t nwaves, void* stream)
{
    if (!v || !out_v || nwaves < 0 || nwaves > (1 << 24)) return EAMRL_E_ARG;
    if (fn == EAMRL_WPROBE_ARGMAX && (!idx || !out_i)) return EAMRL_E_ARG;
    if ((fn == EAMRL_WPROBE_ZROT || fn == EAMRL_WPROBE_Z_TOTAL_REL) && !idx) return EAMRL_E_ARG;
    if (nwaves == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    switch (fn) {
#define EAMRL_CASE(F) case F: return launch_wave<F>(v, idx, out_v, out_i, nwaves, st)
        EAMRL_CASE(EAMRL_WPROBE_TREE_SUM); EAMRL_CASE(EAMRL_WPROBE_MAX); EAMRL_CASE(EAMRL_WPROBE_ARGMAX);
        EAMRL_CASE(EAMRL_WPROBE_VMAX); EAMRL_CASE(EAMRL_WPROBE_VMAX3); EAMRL_CASE(EAMRL_WPROBE_VMAX5);
        EAMRL_CASE(EAMRL_WPROBE_ZROT); EAMRL_CASE(EAMRL_WPROBE_Z_TOTAL_REL);
#undef EAMRL_CASE
    }
    return EAMRL_E_ARG;
}

}  // extern "C"
