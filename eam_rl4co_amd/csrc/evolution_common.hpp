// The fork's EA.run (rl4co/models/zoo/earl/evolution.py:252-354; elitism_selection :1103-1108) once, for every env:
// one workgroup per problem instance runs G generations of select / crossover / mutate / fitness / replace in LDS
// (population and offspring as int16 rows, fitness as fp32); nothing but the final population goes back to HBM.
// The reference draws random numbers inside the operators (numba's per-thread generators); here every draw is an
// input (see eamrl.h), which is what makes the operators reproducible and testable.
//
// k_ea<Ops> is the generation loop; an env supplies its operators as a policy type Ops (evolution_routes.hpp: TSP, CVRP,
// launched from evolution.hip; evolution_prize.hip: PCTSP, OP) with
//   ENV_FLOATS, tail_bytes(O) ... LDS the env wants for itself: floats after `loc`, bytes after `tmp`
//   INIT_MUTATE ................. whether EA.run mutates the initial population (every env but TSP)
//   load(a, b, env, tail, loc, lane)  per-instance arrays into the env's LDS, per-thread constants (runs before the
//                                     first barrier, so it reads its inputs from global memory only)
//   init_mutate(a, row, i) ...... mutation of initial row i = b * S + s          (only if INIT_MUTATE)
//   child(a, p1, p2, role, o, dp, tid) -> keep_parent      the crossover of pair draw dp; p1 / p2 in pair order
//   mutate(a, o, dm) ............ the mutation of offspring draw dm
//   fitness(row, lane) .......... by one wavefront, every lane gets the value
// Every hook is __forceinline__ and Ops holds scalars and LDS pointers only, so it lives in registers.
// The per-offspring rule (ea_offspring) and the order of a sort (ea_before) are functions of their own: the phase kernels of
// evolution_large.hip, which run the same loop on populations in device memory, call them too.
// Sorting is stable ascending (ties keep index order) where the reference leaves tie order to numpy's argsort.
#pragma once
#include "tour_row.hpp"

namespace eamrl {

namespace {

constexpr int EVB = 256;       // threads
constexpr int EV_MAX = 128;    // max population size and node count (rows: 128, CVRP 256)

// One argument block for all envs; a launcher fills what its env reads and leaves the rest null.
struct EaArgs {
    const float* locs; int64_t* pop; float* fitness;
    int64_t B; int S, N, M, L, G, top_k;          // N customers / TSP nodes, M rows of locs, L row length (TSP: N)
    double mutation_rate, crossover_rate;
    const double* cross_rand; const double* mut_rand;             // [G,B,P], [G,B,O]
    int ne, P;     // elites, crossover pairs (host-computed with the reference's integer rules)
    const int32_t* cross_idx; const int32_t* mut_idx;             // TSP: [G,B,P,2], [G,B,O,2]
    const float* demand; const float* vcap;                       // CVRP: [B,N], [B]
    const float* prize; const float* aux;                         // aux: PCTSP penalty [B,M], OP max_length [B,M]
    const double* init_mut_rand; const double* init_mut_u;        // [B,S], [B,S,w]      w = 3 (CVRP), 2 (PCTSP, OP)
    const double* cross_u; const double* mut_u;                   // [G,B,P] (CVRP, OP), [G,B,O,w]
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// np.random.randint(lo, hi) from a uniform u in [0, 1): lo + min(floor(u * (hi - lo)), hi - lo - 1)
__device__ __forceinline__ int rint_u(int lo, int hi, double u)
{
    const int n = hi - lo;
    int k = (int)(u * (double)n);
    k = k > n - 1 ? n - 1 : (k < 0 ? 0 : k);
    return lo + k;
}

// Node sets of the operators ("already in the child").  An operator takes its set type as a template parameter and gets an
// empty set from the type's Pool, which the env's Ops carries: Bits128 lives in two registers and its pool is empty;
// BitsLds (up to 1024 nodes, the device-memory path of evolution_large.hip) keeps its words in LDS, one slot per offspring
// being built, because a register array indexed by a node would go to scratch memory.
struct Bits128 {
    struct Pool { __device__ __forceinline__ Bits128 get(int) const { return Bits128{}; } };
    unsigned long long lo = 0ull, hi = 0ull;
    __device__ __forceinline__ bool test(int i) const { return i < 64 ? (lo >> i) & 1ull : (hi >> (i - 64)) & 1ull; }
    __device__ __forceinline__ void set(int i) { if (i < 64) lo |= 1ull << i; else hi |= 1ull << (i - 64); }
    __device__ __forceinline__ void clear(int i) { if (i < 64) lo &= ~(1ull << i); else hi &= ~(1ull << (i - 64)); }
    __device__ __forceinline__ bool any() const { return (lo | hi) != 0ull; }
    __device__ __forceinline__ int lowest() const { return lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll(hi); }
    __device__ __forceinline__ int count() const { return __builtin_popcountll(lo) + __builtin_popcountll(hi); }
};

struct BitsLds {
    static constexpr int WORDS = 16;               // 1024 nodes
    struct Pool {
        unsigned long long* words;                 // [slots][WORDS] in LDS
        __device__ __forceinline__ BitsLds get(int slot) const
        {
            BitsLds s{words + slot * WORDS};
            for (int i = 0; i < WORDS; ++i) s.w[i] = 0ull;
            return s;
        }
    };
    unsigned long long* w;
    __device__ __forceinline__ bool test(int i) const { return (w[i >> 6] >> (i & 63)) & 1ull; }
    __device__ __forceinline__ void set(int i) { w[i >> 6] |= 1ull << (i & 63); }
    __device__ __forceinline__ int count() const
    {
        int n = 0;
        for (int i = 0; i < WORDS; ++i) n += __builtin_popcountll(w[i]);
        return n;
    }
};

// reverse o[lo..hi]
__device__ __forceinline__ void reverse_row(int16_t* o, int lo, int hi)
{
    for (; lo < hi; ++lo, --hi) { const int16_t x = o[lo]; o[lo] = o[hi]; o[hi] = x; }
}

// Wavefront sums over an int16 row in LDS: the leg of env_rule.hpp in the chunked lane-tree order of tour_row.hpp, identical to
// eamrl_tour_length; every lane gets the result.
// open TSP cycle of row `tour` (int16 [N])
__device__ __forceinline__ float wave_tour_length(const int16_t* tour, const float2* loc, int N, int lane)
{
    return chunked_tree_sum(N, lane, [&](int t) {
        const float2 p0 = loc[tour[t]], p1 = loc[tour[(t + 1 == N) ? 0 : t + 1]];
        return rule::leg(p1.x, p1.y, p0.x, p0.y);
    });
}

// closed tour depot -> row -> depot (L + 1 legs)
__device__ __forceinline__ float wave_route_length(const int16_t* row, const float2* loc, int L, int lane)
{
    return chunked_tree_sum(L + 1, lane, [&](int t) {
        const float2 p0 = loc[t == 0 ? 0 : row[t - 1]], p1 = loc[t == L ? 0 : row[t]];
        return rule::leg(p1.x, p1.y, p0.x, p0.y);
    });
}

// lane tree over v[row[t]], t < L
__device__ __forceinline__ float wave_gather_sum(const int16_t* row, const float* v, int L, int lane)
{
    return chunked_tree_sum(L, lane, [&](int t) { return v[row[t]]; });
}

// bytes of the carve in k_ea without the three populations and the env's tail
template <class Ops>
constexpr size_t ea_fixed_lds()
{
    return EV_MAX * sizeof(float2) + (Ops::ENV_FLOATS + 2 * EV_MAX) * sizeof(float) + 5 * EV_MAX * sizeof(int16_t) + 16;
}

// stable ascending order (ties keep index order): does candidate j come before candidate i?
__device__ __forceinline__ int ea_before(float fj, int j, float fi, int i) { return (fj < fi) | ((fj == fi) & (j < i)); }

// Offspring t = 2 p + role of generation g of instance b, by one thread: the crossover of pair p (p1 / p2 in pair order; pair 0
// always crosses, the others with the adjusted rate) or a copy of the offspring's own parent, then the mutation.  Draws are
// indexed dp = (g B + b) P + p and dm = (g B + b) O + t.  slot: what Ops::child gets as the thread's scratch slot.
template <class Ops>
__device__ __forceinline__ void ea_offspring(const Ops& ops, const EaArgs& a, int g, int64_t b, int t, const int16_t* p1,
                                             const int16_t* p2, int16_t* o, int slot)
{
    const int L = a.L, P = a.P, O = 2 * a.P;
    const int p = t >> 1, role = t & 1;
    const int16_t* own = role ? p2 : p1;
    const int64_t dp = ((int64_t)g * a.B + b) * P + p;
    double rate = a.crossover_rate;
    if (p > 0 && P > 1) {
        rate = ((double)P * a.crossover_rate - 1.0) / (double)(P - 1);
        rate = rate > 1.0 ? 1.0 : rate;
        rate = rate < 0.0 ? 0.0 : rate;
    }
    const double r = (p == 0) ? 0.0 : a.cross_rand[dp];
    bool keep_parent = !(r < rate);
    if (!keep_parent) keep_parent = ops.child(a, p1, p2, role, o, dp, slot);
    if (keep_parent) for (int j = 0; j < L; ++j) o[j] = own[j];
    const int64_t dm = ((int64_t)g * a.B + b) * O + t;
    if (a.mut_rand[dm] < a.mutation_rate) ops.mutate(a, o, dm);
}

template <class Ops>
__global__ __launch_bounds__(EVB) void k_ea(EaArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = a.S, L = a.L, M = a.M, O = 2 * a.P;
    float2* loc = reinterpret_cast<float2*>(smem);                        // [M <= 128]
    float* env = reinterpret_cast<float*>(loc + EV_MAX);                  // [Ops::ENV_FLOATS] the env's own arrays
    float* fit = env + Ops::ENV_FLOATS;                                   // [S]
    float* ofit = fit + EV_MAX;                                           // [O]
    int16_t* first = reinterpret_cast<int16_t*>(ofit + EV_MAX);           // [S] first node of position s
    int16_t* order = first + EV_MAX;                                      // [S + O] sort scratch
    int16_t* sel = order + 2 * EV_MAX;                                    // [ne]
    int* flags = reinterpret_cast<int*>(sel + EV_MAX);                    // [0] duplicate first nodes
    int16_t* pop = reinterpret_cast<int16_t*>(flags + 4);                 // [S][L]
    int16_t* off = pop + (size_t)S * L;                                   // [O][L]
    int16_t* tmp = off + (size_t)S * L;                                   // [S][L] (top-k replacement only)
    uint8_t* tail = reinterpret_cast<uint8_t*>(tmp + (size_t)S * L);      // [Ops::tail_bytes(O)]

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t b = blockIdx.x;

    // ---- load the instance ------------------------------------------------------------------------------------------
    Ops ops;
    ops.load(a, b, env, tail, loc, lane);
    for (int i = tid; i < M; i += EVB) loc[i] = *reinterpret_cast<const float2*>(a.locs + (b * M + i) * 2);
    for (int i = tid; i < S * L; i += EVB) pop[i] = (int16_t)clampi((int)a.pop[b * S * L + i], 0, M - 1);
    if (tid == 0) flags[0] = 0;
    __syncthreads();
    if (tid < S) {
        first[tid] = pop[tid * L];                                        // node_to_position uses the INITIAL first nodes
        if constexpr (Ops::INIT_MUTATE)
            if (a.init_mut_rand[b * S + tid] < a.mutation_rate) ops.init_mutate(a, pop + tid * L, b * S + tid);
    }
    __syncthreads();
    for (int s = wv; s < S; s += EVB / 64) {
        const float f = ops.fitness(pop + s * L, lane);
        if (lane == 0) fit[s] = f;
    }
    if (tid < S) {
        int dup = 0;
        for (int j = 0; j < tid; ++j) dup |= (first[j] == first[tid]);
        if (dup) atomicOr(&flags[0], 1);
    }
    __syncthreads();
    const bool by_first = flags[0] == 0 && !a.top_k;

    for (int g = 0; g < a.G && O > 0; ++g) {
        // ---- select: the ne fittest, in ascending fitness order (stable) ----------------------------------------------
        if (S <= 2) {
            if (tid < S) sel[tid] = (int16_t)tid;
        } else if (tid < S) {
            const float f = fit[tid];
            int rank = 0;
            for (int j = 0; j < S; ++j) rank += ea_before(fit[j], j, f, tid);
            if (rank >= S - a.ne) sel[rank - (S - a.ne)] = (int16_t)tid;
        }
        __syncthreads();

        // ---- crossover + mutation: thread t builds offspring t of pair t / 2 -----------------------------------------
        if (tid < O) {
            const int p = tid >> 1;
            ea_offspring(ops, a, g, b, tid, pop + (int)sel[2 * p] * L, pop + (int)sel[2 * p + 1] * L, off + tid * L, tid);
        }
        __syncthreads();

        // ---- fitness of the offspring -----------------------------------------------------------------------------------
        for (int t = wv; t < O; t += EVB / 64) {
            const float f = ops.fitness(off + t * L, lane);
            if (lane == 0) ofit[t] = f;
        }
        __syncthreads();

        // ---- replacement ----------------------------------------------------------------------------------------------
        if (by_first) {
            // position s keeps the best of pop[s] and the offspring starting at its node; earliest wins ties
            if (tid < S) {
                float best = fit[tid];
                int src = -1;
                for (int t = 0; t < O; ++t)
                    if (off[t * L] == first[tid] && ofit[t] > best) { best = ofit[t]; src = t; }
                order[tid] = (int16_t)src;
                if (src >= 0) fit[tid] = best;
            }
            __syncthreads();
            for (int i = tid; i < S * L; i += EVB) {
                const int s = i / L, src = order[s];
                if (src >= 0) pop[i] = off[src * L + (i - s * L)];
            }
        } else {
            // the S fittest of pop ++ offspring, descending = reversed stable ascending order
            const int C = S + O;
            if (tid < C) {
                const float f = tid < S ? fit[tid] : ofit[tid - S];
                int rank = 0;
                for (int j = 0; j < C; ++j) {
                    const float fj = j < S ? fit[j] : ofit[j - S];
                    rank += ea_before(fj, j, f, tid);
                }
                order[tid] = (int16_t)(C - 1 - rank);           // position in descending order
            }
            __syncthreads();
            for (int i = tid; i < C * L; i += EVB) {
                const int c = i / L, dst = order[c];
                if (dst < S) tmp[dst * L + (i - c * L)] = c < S ? pop[i] : off[i - S * L];
            }
            float keep = 0.0f;
            int dst = S;
            if (tid < C) { dst = order[tid]; keep = tid < S ? fit[tid] : ofit[tid - S]; }
            __syncthreads();
            if (dst < S) fit[dst] = keep;
            for (int i = tid; i < S * L; i += EVB) pop[i] = tmp[i];
        }
        __syncthreads();
    }

    for (int i = tid; i < S * L; i += EVB) a.pop[b * S * L + i] = pop[i];
    if (tid < S) a.fitness[b * S + tid] = fit[tid];
}

// the launch of every env: elite and pair counts, LDS size and its limits
template <class Ops>
int ea_launch(EaArgs a, double selection_rate, hipStream_t st)
{
    a.ne = ea_num_elites(selection_rate, a.S);
    a.P = a.ne / 2;
    const size_t lds = ea_fixed_lds<Ops>() + 3 * (size_t)a.S * a.L * sizeof(int16_t) + Ops::tail_bytes(2 * a.P);
    if (lds > 150 * 1024) return EAMRL_E_ARG;
    auto k = k_ea<Ops>;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return EAMRL_E_LAUNCH;
    hipLaunchKernelGGL(k, dim3((unsigned)a.B), dim3(EVB), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

}  // namespace

}  // namespace eamrl
