// TSP and CVRP operators of the evolutionary improvement of tour populations (the fork's EA.run), stated once for both
// execution paths: k_ea of evolution_common.hpp (populations in LDS, node sets Bits128; launched from evolution.hip) and the
// phase kernels of evolution_large.hip (populations in device memory, node sets BitsLds).  The set type is a template
// parameter of the operators and of TspOps / CvrpOps; the Bits128 instantiation is k_ea's code.
//
// Reference (numba on CPU threads, one Python thread per instance):
//   calculate_fitness_tsp .... rl4co/models/zoo/earl/evolution.py:356-362
//   order_crossover_tsp ...... :392-488     inverse_mutate_tsp .... :490-517
//   calculate_fitness_cvrp ... :364-370     order_crossover_cvrp .. :585-788     inverse_mutate_cvrp ... :519-553
//
// Integer results are bit-exact against oracle/ea_oracle.py.  Fitness uses the canonical tour length
// (sqrtf(fmaf(dy,dy,dx*dx)) per leg, lane tree over legs), identical to eamrl_tour_length.
#pragma once
#include "evolution_common.hpp"

namespace eamrl {

namespace {

// ---- TSP --------------------------------------------------------------------------------------------------------------
// order_crossover_tsp: own[0] and own[start, end) stay in place, the other positions take `other`'s nodes in order,
// from `end` on.  No "keep the parent" outcome.
// `used`: an empty set.
template <class Set>
__device__ __forceinline__ void tsp_order_crossover(const int16_t* own, const int16_t* other, int16_t* o, int N, int i1, int i2,
                                                    Set used)
{
    const int start = i1 < i2 ? i1 : i2, end = i1 < i2 ? i2 : i1;
    for (int i = 0; i < N; ++i) o[i] = -1;
    o[0] = own[0];
    used.set(own[0]);
    for (int i = start; i < end; ++i) { o[i] = own[i]; used.set(own[i]); }
    int pos = end % N, j = 0;
    for (int it = 0; it < N; ++it) {
        if (pos != 0 && o[pos] == -1) {
            while (j < N && used.test(other[j])) ++j;      // first node of `other` not yet in the child
            if (j < N) { o[pos] = other[j]; used.set(other[j]); ++j; }
        }
        pos = (pos + 1 == N) ? 0 : pos + 1;
    }
    for (int i = 0; i < N; ++i) if (o[i] < 0) o[i] = 0;   // only reachable with non-permutation input
}

// inverse_mutate_tsp: reverse o[start, end); an empty range swaps with the next node
__device__ __forceinline__ void tsp_inverse_mutate(int16_t* o, int N, int i1, int i2)
{
    const int start = i1 < i2 ? i1 : i2, end = i1 < i2 ? i2 : i1;
    if (start < end) reverse_row(o, start, end - 1);
    else if (start < N - 1) reverse_row(o, start, start + 1);
}

template <class Set>
struct TspOps {
    static constexpr int ENV_FLOATS = 0;
    static constexpr bool INIT_MUTATE = false;
    static constexpr size_t tail_bytes(int) { return 0; }
    const float2* loc; int N; float worst;
    typename Set::Pool sets;
    template <int THREADS = EVB>
    __device__ __forceinline__ void load(const EaArgs& a, int64_t, float*, uint8_t*, const float2* loc_, int)
    {
        loc = loc_; N = a.N; worst = (float)(1.5 * (double)N);
    }
    __device__ __forceinline__ bool child(const EaArgs& a, const int16_t* p1, const int16_t* p2, int role, int16_t* o,
                                          int64_t dp, int slot) const
    {
        tsp_order_crossover(role ? p2 : p1, role ? p1 : p2, o, N, clampi(a.cross_idx[2 * dp], 1, N - 1),
                            clampi(a.cross_idx[2 * dp + 1], 1, N - 1), sets.get(slot));
        return false;
    }
    __device__ __forceinline__ void mutate(const EaArgs& a, int16_t* o, int64_t dm) const
    {
        tsp_inverse_mutate(o, N, clampi(a.mut_idx[2 * dm], 1, N - 1), clampi(a.mut_idx[2 * dm + 1], 1, N - 1));
    }
    __device__ __forceinline__ float fitness(const int16_t* row, int lane) const { return worst - wave_tour_length(row, loc, N, lane); }
};

// ---- CVRP -------------------------------------------------------------------------------------------------------------
// inverse_mutate_cvrp on one row: reverse a random segment strictly inside one route
__device__ __forceinline__ void cvrp_mutate_row(int16_t* o, int L, const double* u3)
{
    int depots = 0;
    for (int j = 0; j < L; ++j) depots += (o[j] == 0);
    if (depots <= 1) return;
    const int r = rint_u(0, depots - 1, u3[0]);
    int seen = 0, z0 = -1, z1 = -1;
    for (int j = 0; j < L; ++j) {
        if (o[j] == 0) {
            if (seen == r) z0 = j;
            if (seen == r + 1) { z1 = j; break; }
            ++seen;
        }
    }
    const int start = z0 + 1, end = z1 - 1;
    if (end - start > 1) {
        const int s0 = rint_u(start, end, u3[1]);
        const int s1 = rint_u(s0 + 1, end + 1, u3[2]);
        reverse_row(o, s0, s1 - 1);
    }
}

// routes of a parent as the crossover counts them: zeros before the last non-zero entry
__device__ __forceinline__ int cvrp_route_num(const int16_t* par, int L)
{
    int valid_end = 1;
    for (int j = L - 1; j >= 0; --j) if (par[j] != 0) { valid_end = j + 1; break; }
    int zeros = 0;
    for (int j = 0; j < valid_end; ++j) zeros += (par[j] == 0);
    return zeros;
}

// One child of order_crossover_cvrp: `own`'s routes up to a random cut, then the customers they miss in index order, a
// new route whenever the load would exceed the capacity.  true = keep the parent.  `used`: an empty set.
template <class Set>
__device__ __forceinline__ bool cvrp_child(const int16_t* own, const int16_t* other, int16_t* o, int N, int L, const float* dem,
                                           double vcap, double u, Set used)
{
    const int m0 = cvrp_route_num(own, L), m1 = cvrp_route_num(other, L);
    const int m = m0 < m1 ? m0 : m1;
    const int end = m > 1 ? rint_u(1, m, u) : 0;
    int end_idx = 0;
    if (end > 0) {
        int seen = 0;
        for (int j = 0; j < L; ++j) if (own[j] == 0) { if (seen == end) { end_idx = j; break; } ++seen; }
    }
    bool dz = false;                               // two consecutive depot visits somewhere in the child
    int pos = 0, last = -1;
    auto push = [&](int x) {
        if (pos < L) o[pos] = (int16_t)x;
        if (pos >= 1 && x == 0 && last == 0) dz = true;
        last = x;
        ++pos;
    };
    for (int j = 0; j < end_idx; ++j) {
        const int x = own[j];
        if (x > 0) used.set(x);
        push(x);
    }
    if (pos > 0 && last != 0) push(0);
    const int count = N - used.count();
    double load = 0.0;
    int i = 0, first_unused = 0;
    for (int node = 1; node <= N; ++node) {
        if (used.test(node)) continue;
        if (first_unused == 0) first_unused = node;
        if (pos >= 2 * L - 1) break;
        const double d = (double)dem[node - 1];
        if (load + d > vcap) {
            if (pos > 0 && last == 0 && i < count - 1) { ++i; continue; }
            push(0);
            load = 0.0;
            if (pos >= 2 * L - 1) break;
        }
        push(node);
        load += d;
        ++i;
    }
    if (pos < 2 * L && last != 0) {
        // the reference's "all visited" test never sees the nodes it just appended: it fails exactly when
        // the smallest customer missing from the copied prefix has an index below the number of missing ones
        if (first_unused == 0)
            for (int node = 1; node <= N && first_unused == 0; ++node)
                if (!used.test(node)) first_unused = node;
        const bool all_visited = (count == 0) || !(first_unused < count);
        if (all_visited) push(0);
    }
    if ((dz && count > 0) || pos - 1 >= L) return true;
    for (int j = pos; j < L; ++j) o[j] = 0;
    return false;
}

template <class Set>
struct CvrpOps {
    static constexpr int ENV_FLOATS = EV_MAX;      // dem [N] (k_ea's carve; the large path sizes its own)
    static constexpr bool INIT_MUTATE = true;
    static constexpr size_t tail_bytes(int) { return 0; }
    const float2* loc; float* dem; double vcap; int N, L; float worst;
    typename Set::Pool sets;
    template <int THREADS = EVB>      // of the workgroup that loads
    __device__ __forceinline__ void load(const EaArgs& a, int64_t b, float* env, uint8_t*, const float2* loc_, int)
    {
        loc = loc_; dem = env; N = a.N; L = a.L;
        worst = (float)(2.5 * (double)L);
        vcap = (double)a.vcap[b];
        for (int i = threadIdx.x; i < N; i += THREADS) dem[i] = a.demand[b * N + i];
    }
    __device__ __forceinline__ void init_mutate(const EaArgs& a, int16_t* row, int64_t i) const { cvrp_mutate_row(row, L, a.init_mut_u + i * 3); }
    __device__ __forceinline__ bool child(const EaArgs& a, const int16_t* p1, const int16_t* p2, int role, int16_t* o,
                                          int64_t dp, int slot) const
    {
        return cvrp_child(role ? p2 : p1, role ? p1 : p2, o, N, L, dem, vcap, a.cross_u[dp], sets.get(slot));
    }
    __device__ __forceinline__ void mutate(const EaArgs& a, int16_t* o, int64_t dm) const { cvrp_mutate_row(o, L, a.mut_u + dm * 3); }
    __device__ __forceinline__ float fitness(const int16_t* row, int lane) const { return worst - wave_route_length(row, loc, L, lane); }
};

}  // namespace

}  // namespace eamrl
