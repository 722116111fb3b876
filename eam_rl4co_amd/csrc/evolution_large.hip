// The device-memory path of the TSP and CVRP evolutionary improvement (the fork's EA.run, rl4co/models/zoo/earl/
// evolution.py:252-354) for populations and graphs of up to 1024: the same generation loop as k_ea (evolution_common.hpp),
// the same operators (evolution_routes.hpp, on BitsLds node sets) and the same arithmetic and tie rules, but the three
// populations live in a caller-supplied scratch buffer and every phase is a launch of its own, so that the few instances of
// a large-graph batch spread over the whole device:
//
//   k_eal_init ....... (instance, 4 rows)      int64 pop -> int16 rows, initial first nodes, initial mutation (CVRP), fitness
//                                              by one wavefront per row, the instance's duplicate-first-node flag
//   per generation
//   k_eal_select ..... (instance)              the ne fittest in stable ascending order
//   k_eal_offspring .. (instance, pair)        64 threads: parents and children staged in LDS, lane 0 / lane 1 build the two
//                                              children with ea_offspring, the wavefront computes both fitnesses
//   k_eal_rank ....... (instance)              per-first-node: the source offspring of every position; top-k: the place of
//                                              every candidate in the descending order; the new fitness
//   k_eal_move ....... (instance, candidate)   rows to their new place (top-k: into tmp)
//   k_eal_settle ..... (instance, row)         top-k only: tmp -> pop
//   k_eal_final ...... (instance, row)         int16 -> int64 back into the caller's pop, fitness out
//
// The launch boundary is the only synchronisation between phases: no kernel waits for another workgroup, every loop is
// bounded by N, L, S or G, and the library neither allocates nor synchronises.
#include "evolution_routes.hpp"

namespace eamrl {

namespace {

constexpr int EVL_MAX = 1024;      // max population size and node count
constexpr int EVL_ROWS = 4;        // rows (wavefronts) per workgroup of k_eal_init

// The scratch carve, all instances of one kind together; O is bounded by S, so one buffer serves every selection rate.
struct EaScratch {
    float* fit; float* ofit;             // [B][S], [B][S]
    int* dup;                            // [B] duplicate first nodes in the initial population
    int16_t* pop; int16_t* off; int16_t* tmp;      // [B][S][L] each (off: the first O rows)
    int16_t* first; int16_t* sel;        // [B][S] initial first node of position s; [B][S] the elites (first ne)
    int16_t* order;                      // [B][2 S] per-first-node: source offspring of position s or -1; top-k: new place
};

size_t scratch_carve(void* base, int64_t B, int S, int L, EaScratch* sc)
{
    const size_t rows = (size_t)B * S, cells = rows * L;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t q = at; at += (bytes + 15) & ~(size_t)15; return q; };
    const size_t fit = take(rows * sizeof(float)), ofit = take(rows * sizeof(float)), dup = take((size_t)B * sizeof(int));
    const size_t pop = take(cells * sizeof(int16_t)), off = take(cells * sizeof(int16_t)), tmp = take(cells * sizeof(int16_t));
    const size_t first = take(rows * sizeof(int16_t)), sel = take(rows * sizeof(int16_t)), order = take(2 * rows * sizeof(int16_t));
    if (sc) {
        char* p = static_cast<char*>(base);
        auto f32 = [&](size_t o) { return reinterpret_cast<float*>(p + o); };
        auto i16 = [&](size_t o) { return reinterpret_cast<int16_t*>(p + o); };
        *sc = EaScratch{f32(fit), f32(ofit), reinterpret_cast<int*>(p + dup), i16(pop), i16(off), i16(tmp), i16(first), i16(sel),
                        i16(order)};
    }
    return at;
}

// LDS of a workgroup that stages `rows` rows, the coordinates and (CVRP) the demands
template <class Ops>
__host__ __device__ constexpr size_t staged_lds(int rows, int L, int M)
{
    return (size_t)M * sizeof(float2) + (Ops::INIT_MUTATE ? (size_t)M * sizeof(float) : 0) + (size_t)rows * L * sizeof(int16_t);
}

template <class Ops>
__global__ __launch_bounds__(EVB) void k_eal_init(EaArgs a, EaScratch sc)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int seen[EVL_MAX];
    const int S = a.S, L = a.L, M = a.M;
    float2* loc = reinterpret_cast<float2*>(smem);                                   // [M]
    float* env = reinterpret_cast<float*>(loc + M);                                  // [M] if the env has demands
    int16_t* rows = reinterpret_cast<int16_t*>(env + (Ops::INIT_MUTATE ? M : 0));    // [EVL_ROWS][L]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t b = blockIdx.x;
    const int s = blockIdx.y * EVL_ROWS + wv;
    int16_t* row = rows + wv * L;

    Ops ops;
    ops.template load<EVB>(a, b, env, nullptr, loc, lane);
    for (int i = tid; i < M; i += EVB) loc[i] = *reinterpret_cast<const float2*>(a.locs + (b * M + i) * 2);
    if (s < S)
        for (int j = lane; j < L; j += 64) row[j] = (int16_t)clampi((int)a.pop[(b * S + s) * L + j], 0, M - 1);
    if (blockIdx.y == 0) for (int i = tid; i < EVL_MAX; i += EVB) seen[i] = 0;
    __syncthreads();
    if (s < S && lane == 0) {
        sc.first[b * S + s] = row[0];                                     // node_to_position uses the INITIAL first nodes
        if constexpr (Ops::INIT_MUTATE)
            if (a.init_mut_rand[b * S + s] < a.mutation_rate) ops.init_mutate(a, row, b * S + s);
    }
    if (blockIdx.y == 0) {
        // two positions share a first node exactly when some node is counted twice
        int dup = 0;
        for (int i = tid; i < S; i += EVB)
            dup |= atomicAdd(&seen[clampi((int)a.pop[(b * S + i) * L], 0, M - 1)], 1) > 0;
        dup = __syncthreads_or(dup);
        if (tid == 0) sc.dup[b] = dup;
    }
    __syncthreads();
    if (s < S) {
        const float f = ops.fitness(row, lane);
        if (lane == 0) sc.fit[b * S + s] = f;
        for (int j = lane; j < L; j += 64) sc.pop[(b * S + s) * L + j] = row[j];
    }
}

// the ne fittest, in ascending fitness order (stable)
__global__ __launch_bounds__(EVB) void k_eal_select(EaArgs a, EaScratch sc)
{
    __shared__ float fit[EVL_MAX];
    const int S = a.S, tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    for (int i = tid; i < S; i += EVB) fit[i] = sc.fit[b * S + i];
    __syncthreads();
    for (int i = tid; i < S; i += EVB) {
        if (S <= 2) { sc.sel[b * S + i] = (int16_t)i; continue; }
        const float f = fit[i];
        int rank = 0;
        for (int j = 0; j < S; ++j) rank += ea_before(fit[j], j, f, i);
        if (rank >= S - a.ne) sc.sel[b * S + rank - (S - a.ne)] = (int16_t)i;
    }
}

template <class Ops>
__global__ __launch_bounds__(64) void k_eal_offspring(EaArgs a, EaScratch sc, int g)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ unsigned long long setw[2 * BitsLds::WORDS];
    const int S = a.S, L = a.L, M = a.M;
    float2* loc = reinterpret_cast<float2*>(smem);                                   // [M]
    float* env = reinterpret_cast<float*>(loc + M);                                  // [M] if the env has demands
    int16_t* rows = reinterpret_cast<int16_t*>(env + (Ops::INIT_MUTATE ? M : 0));    // parents 0 1, children 2 3: [4][L]
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int p = blockIdx.y;

    Ops ops;
    ops.template load<64>(a, b, env, nullptr, loc, lane);
    ops.sets.words = setw;
    for (int i = lane; i < M; i += 64) loc[i] = *reinterpret_cast<const float2*>(a.locs + (b * M + i) * 2);
    for (int r = 0; r < 2; ++r) {
        const int16_t* src = sc.pop + (b * S + sc.sel[b * S + 2 * p + r]) * L;
        for (int j = lane; j < L; j += 64) rows[r * L + j] = src[j];
    }
    __syncthreads();
    if (lane < 2) ea_offspring(ops, a, g, b, 2 * p + lane, rows, rows + L, rows + (2 + lane) * L, lane);
    __syncthreads();
    for (int r = 0; r < 2; ++r) {
        const int16_t* child = rows + (2 + r) * L;
        const int64_t t = b * S + 2 * p + r;
        const float f = ops.fitness(child, lane);
        if (lane == 0) sc.ofit[t] = f;
        for (int j = lane; j < L; j += 64) sc.off[t * L + j] = child[j];
    }
}

// by_first of k_ea: the first nodes of the initial population are pairwise distinct and the caller did not ask for top-k
__device__ __forceinline__ bool by_first_node(const EaArgs& a, const EaScratch& sc, int64_t b) { return sc.dup[b] == 0 && !a.top_k; }

__global__ __launch_bounds__(EVB) void k_eal_rank(EaArgs a, EaScratch sc)
{
    __shared__ float cf[2 * EVL_MAX];           // fitness of the candidates: population, then offspring
    __shared__ int16_t ofirst[EVL_MAX];         // first node of every offspring
    const int S = a.S, L = a.L, O = 2 * a.P, C = S + O, tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    for (int i = tid; i < C; i += EVB) cf[i] = i < S ? sc.fit[b * S + i] : sc.ofit[b * S + i - S];
    for (int t = tid; t < O; t += EVB) ofirst[t] = sc.off[(b * S + t) * L];
    __syncthreads();
    if (by_first_node(a, sc, b)) {
        // position s keeps the best of pop[s] and the offspring starting at its node; earliest wins ties
        for (int s = tid; s < S; s += EVB) {
            const int16_t first = sc.first[b * S + s];
            float best = cf[s];
            int src = -1;
            for (int t = 0; t < O; ++t)
                if (ofirst[t] == first && cf[S + t] > best) { best = cf[S + t]; src = t; }
            sc.order[b * 2 * S + s] = (int16_t)src;
            if (src >= 0) sc.fit[b * S + s] = best;
        }
    } else {
        // the S fittest of pop ++ offspring, descending = reversed stable ascending order
        for (int c = tid; c < C; c += EVB) {
            const float f = cf[c];
            int rank = 0;
            for (int j = 0; j < C; ++j) rank += ea_before(cf[j], j, f, c);
            const int dst = C - 1 - rank;
            sc.order[b * 2 * S + c] = (int16_t)dst;
            if (dst < S) sc.fit[b * S + dst] = f;
        }
    }
}

__global__ __launch_bounds__(EVB) void k_eal_move(EaArgs a, EaScratch sc)
{
    const int S = a.S, L = a.L, tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int c = blockIdx.y;                   // candidate: position c < S, offspring c - S
    const int16_t* src;
    int16_t* dst;
    if (by_first_node(a, sc, b)) {
        if (c >= S) return;
        const int t = sc.order[b * 2 * S + c];
        if (t < 0) return;
        src = sc.off + (b * S + t) * L;
        dst = sc.pop + (b * S + c) * L;
    } else {
        const int d = sc.order[b * 2 * S + c];
        if (d >= S) return;
        src = c < S ? sc.pop + (b * S + c) * L : sc.off + (b * S + c - S) * L;
        dst = sc.tmp + (b * S + d) * L;
    }
    for (int j = tid; j < L; j += EVB) dst[j] = src[j];
}

__global__ __launch_bounds__(EVB) void k_eal_settle(EaArgs a, EaScratch sc)
{
    const int64_t b = blockIdx.x, r = b * a.S + blockIdx.y;
    if (by_first_node(a, sc, b)) return;
    for (int j = threadIdx.x; j < a.L; j += EVB) sc.pop[r * a.L + j] = sc.tmp[r * a.L + j];
}

__global__ __launch_bounds__(EVB) void k_eal_final(EaArgs a, EaScratch sc)
{
    const int64_t r = (int64_t)blockIdx.x * a.S + blockIdx.y;
    for (int j = threadIdx.x; j < a.L; j += EVB) a.pop[r * a.L + j] = sc.pop[r * a.L + j];
    if (threadIdx.x == 0) a.fitness[r] = sc.fit[r];
}

template <class Ops>
int ea_launch_large(EaArgs a, double selection_rate, void* scratch, size_t scratch_bytes, hipStream_t st)
{
    a.ne = ea_num_elites(selection_rate, a.S);
    a.P = a.ne / 2;
    EaScratch sc;
    if (a.S > EVL_MAX || a.M > EVL_MAX || scratch_carve(scratch, a.B, a.S, a.L, &sc) > scratch_bytes) return EAMRL_E_ARG;
    const unsigned B = (unsigned)a.B, S = (unsigned)a.S, O = 2u * (unsigned)a.P;
    hipLaunchKernelGGL(k_eal_init<Ops>, dim3(B, (S + EVL_ROWS - 1) / EVL_ROWS), dim3(EVB), staged_lds<Ops>(EVL_ROWS, a.L, a.M), st,
                       a, sc);
    for (int g = 0; g < a.G && O > 0; ++g) {
        hipLaunchKernelGGL(k_eal_select, dim3(B), dim3(EVB), 0, st, a, sc);
        hipLaunchKernelGGL(k_eal_offspring<Ops>, dim3(B, (unsigned)a.P), dim3(64), staged_lds<Ops>(4, a.L, a.M), st, a, sc, g);
        hipLaunchKernelGGL(k_eal_rank, dim3(B), dim3(EVB), 0, st, a, sc);
        hipLaunchKernelGGL(k_eal_move, dim3(B, S + O), dim3(EVB), 0, st, a, sc);
        hipLaunchKernelGGL(k_eal_settle, dim3(B, S), dim3(EVB), 0, st, a, sc);
    }
    hipLaunchKernelGGL(k_eal_final, dim3(B, S), dim3(EVB), 0, st, a, sc);
    return hipGetLastError() == hipSuccess ? 0 : EAMRL_E_LAUNCH;
}

}  // namespace

size_t ea_large_scratch_bytes(int64_t B, int S, int L) { return scratch_carve(nullptr, B, S, L, nullptr); }

int launch_ea_tsp_large(const float* locs, int64_t* pop, float* fitness, int64_t B, int S, int N, int G, double mutation_rate,
                        double crossover_rate, double selection_rate, const double* cross_rand, const int32_t* cross_idx,
                        const double* mut_rand, const int32_t* mut_idx, void* scratch, size_t scratch_bytes, hipStream_t st)
{
    EaArgs a{};
    a.locs = locs; a.pop = pop; a.fitness = fitness; a.B = B; a.S = S; a.N = N; a.M = N; a.L = N; a.G = G;
    a.mutation_rate = mutation_rate; a.crossover_rate = crossover_rate;
    a.cross_rand = cross_rand; a.cross_idx = cross_idx; a.mut_rand = mut_rand; a.mut_idx = mut_idx;
    return ea_launch_large<TspOps<BitsLds>>(a, selection_rate, scratch, scratch_bytes, st);
}

int launch_ea_cvrp_large(const float* locs, const float* demand, const float* vcap, int64_t* pop, float* fitness, int64_t B,
                         int S, int N, int L, int G, double mutation_rate, double crossover_rate, double selection_rate,
                         int top_k, const double* init_mut_rand, const double* init_mut_u, const double* cross_rand,
                         const double* cross_u, const double* mut_rand, const double* mut_u, void* scratch,
                         size_t scratch_bytes, hipStream_t st)
{
    EaArgs a{};
    a.locs = locs; a.demand = demand; a.vcap = vcap; a.pop = pop; a.fitness = fitness;
    a.B = B; a.S = S; a.N = N; a.M = N + 1; a.L = L; a.G = G; a.top_k = top_k;
    a.mutation_rate = mutation_rate; a.crossover_rate = crossover_rate;
    a.init_mut_rand = init_mut_rand; a.init_mut_u = init_mut_u; a.cross_rand = cross_rand; a.cross_u = cross_u;
    a.mut_rand = mut_rand; a.mut_u = mut_u;
    return ea_launch_large<CvrpOps<BitsLds>>(a, selection_rate, scratch, scratch_bytes, st);
}

}  // namespace eamrl
