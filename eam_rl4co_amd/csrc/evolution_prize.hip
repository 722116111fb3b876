// PCTSP and OP operators of the evolutionary improvement of tour populations (the fork's EA.run for the prize-collecting
// envs); the generation loop they plug into is k_ea in evolution_common.hpp.
//
// Reference (numba on CPU threads):
//   inverse_mutate_pctsp ..... rl4co/models/zoo/earl/evolution.py:555-583
//   cycle_crossover_pctsp .... :905-1101     calculate_fitness_cvrp (PCTSP) :364-370
//   order_crossover_op ....... :1110-1346    inverse_mutate_op ...... :1468-1572   calculate_fitness_op .......... :372-378
//
// Arithmetic restated from numba's typing (oracle/ea_oracle.py has the same notes): float32 array elements added to a
// `0.0` accumulator are summed in float64; PCTSP's prize/penalty ratios are rounded to float32 when stored; OP's distance
// matrix is float32 sqrt(dx*dx + dy*dy) with every operation rounded (no fused multiply-add).
// Defined choices: stable ascending sort where the reference leaves ties to numpy's argsort; the cycle crossover's
// `next(iter(set))` starts at the smallest remaining node (slot == value in CPython's and numba's tables for small ints);
// customers the OP crossover would look up beyond the node count (it reads out of bounds there) do not exist.
// Integer results are bit-exact against oracle/ea_oracle.py; fitness uses the canonical reward arithmetic of
// eamrl_pctsp_reward / eamrl_op_reward (lane-tree sums).
#include "evolution_common.hpp"

namespace eamrl {

namespace {

// float32 distance of EA.run's calculate_distance_matrix: sqrt(dx*dx + dy*dy), each operation rounded
__device__ __forceinline__ double dist32(const float2* loc, int a, int b)
{
    const float dx = __fsub_rn(loc[a].x, loc[b].x), dy = __fsub_rn(loc[a].y, loc[b].y);
    return (double)__fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
}

// index after the last non-zero entry at index >= 1; L when there is none
__device__ __forceinline__ int valid_end_from_one(const int16_t* row, int L)
{
    for (int j = L - 1; j >= 1; --j) if (row[j] != 0) return j + 1;
    return L;
}

// ---- PCTSP ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pctsp_mutate_row(int16_t* o, int L, const double* u2)
{
    int v = -1;
    for (int j = L - 1; j >= 0; --j) if (o[j] != 0) { v = j; break; }
    if (v < 2) return;
    const int i1 = rint_u(1, v, u2[0]), i2 = rint_u(1, v, u2[1]);
    const int start = i1 < i2 ? i1 : i2, end = i1 < i2 ? i2 : i1;
    if (start < end) reverse_row(o, start, end - 1);
    else if (start < L - 1) reverse_row(o, start, start + 1);
}

// One child of cycle_crossover_pctsp.  p1 / p2 are the pair's parents IN PAIR ORDER (the cycles are found from p1's side for
// both children); role 0 -> o1, role 1 -> o2.  scratch: 2 * EV_MAX bytes of this thread.
__device__ __forceinline__ void pctsp_child(const int16_t* p1, const int16_t* p2, int role, int16_t* o, int L, int M,
                                            const float* prize, const float* penalty, uint8_t* scratch)
{
    uint8_t* pos2 = scratch;            // [M] position of a node in p2's customer list, 0xFF = absent
    uint8_t* p1c = scratch + EV_MAX;    // [n1] p1's customers in order
    for (int i = 0; i < M; ++i) pos2[i] = 0xFF;
    int e1 = 0, e2 = 0;
    for (int j = L - 1; j >= 0; --j) if (p1[j] != 0) { e1 = j + 1; break; }
    for (int j = L - 1; j >= 0; --j) if (p2[j] != 0) { e2 = j + 1; break; }
    int n1 = 0, n2 = 0;
    Bits128 remaining;
    for (int j = 0; j < e1; ++j) if (p1[j] > 0) { p1c[n1++] = (uint8_t)p1[j]; remaining.set(p1[j]); }
    for (int j = 0; j < e2; ++j) if (p2[j] > 0) pos2[p2[j]] = (uint8_t)n2++;

    Bits128 used;
    double total = 0.0;
    int count = 0;
    auto emit = [&](int node) {
        if (node > 0 && !used.test(node)) {
            if (count < L) o[count] = (int16_t)node;
            ++count;
            used.set(node);
            total += (double)prize[node];
        }
    };
    for (int c = 0; remaining.any(); ++c) {
        const int start = remaining.lowest();
        int node = start;
        while (true) {
            remaining.clear(node);
            // o1 receives every node of every cycle; o2 the whole odd cycles and, of the even ones, the nodes p2 also visits
            if (role == 0 || (c & 1) || pos2[node] != 0xFF) emit(node);
            if (pos2[node] == 0xFF) break;
            const int k = pos2[node];
            if (k >= n1) break;
            node = p1c[k];
            if (node == start || !remaining.test(node)) break;
        }
    }
    const int N = M - 1;
    while (total < 1.0 - 1e-5) {
        int best = 0;
        double best_ratio = -1.0;
        for (int i = 1; i <= N; ++i) {
            if (used.test(i)) continue;
            const float ratio = (float)((double)prize[i] / ((double)penalty[i] + 1e-10));
            if ((double)ratio > best_ratio) { best_ratio = (double)ratio; best = i; }
        }
        if (best == 0) break;
        emit(best);
    }
    for (int j = count < L ? count : L; j < L; ++j) o[j] = 0;
}

// ---- OP ---------------------------------------------------------------------------------------------------------------
// One child of order_crossover_op from `own` with the shared cut `end`; false = keep the parent.
__device__ __forceinline__ bool op_child(const int16_t* own, int end, int16_t* o, int L, int M, const float2* loc,
                                         double global_max)
{
    const double safe = global_max - 0.1;
    Bits128 used;
    for (int j = 0; j < end; ++j) { o[j] = own[j]; if (own[j] != 0) used.set(own[j]); }
    double cur = 0.0;
    for (int j = 1; j < end; ++j) cur += dist32(loc, o[j - 1], o[j]);
    cur += dist32(loc, 0, o[0]);
    int pos = end, last = o[end - 1];
    for (int node = 1; node <= L; ++node) {
        if (node >= M || used.test(node)) continue;
        const double nxt = dist32(loc, last, node), back = dist32(loc, node, 0);
        if (cur + nxt + back <= safe) {
            if (pos < L) o[pos] = (int16_t)node;
            cur += nxt;
            used.set(node);
            last = node;
            ++pos;
        }
        if (pos >= 2 * L - 2) break;
    }
    if (pos >= L) return false;                     // the closing depot visit would land at index >= L
    for (int j = pos; j < L; ++j) o[j] = 0;
    // post-check: closed by a depot visit, legs 1.. within max - 1e-5, no customer twice
    int ve = valid_end_from_one(o, L);
    if (o[ve - 1] != 0) {
        if (ve < L) { o[ve] = 0; ++ve; } else o[ve - 1] = 0;
    }
    double total = 0.0;
    bool dup = false;
    Bits128 seen;
    for (int j = 1; j < ve; ++j) {
        total += dist32(loc, o[j - 1], o[j]);
        if (o[j] != 0) {
            if (seen.test(o[j])) { dup = true; break; }
            seen.set(o[j]);
        }
    }
    return total <= global_max - 1e-5 && !dup;
}

__device__ __forceinline__ void op_mutate_row(int16_t* row, int L, const float2* loc, double global_max, const double* u2)
{
    const double safe = global_max - 1e-5;
    int ve = valid_end_from_one(row, L);
    if (ve <= 3) return;
    int cz = -1;
    int16_t cz_old = 0;
    if (row[ve - 1] != 0) {
        if (ve < L) { cz = ve; cz_old = row[ve]; row[ve] = 0; ++ve; }
        else { cz = ve - 1; cz_old = row[ve - 1]; row[ve - 1] = 0; }
    }
    double cur = dist32(loc, 0, row[0]);
    for (int j = 1; j < ve; ++j) cur += dist32(loc, row[j - 1], row[j]);
    const int s = rint_u(1, ve - 2, u2[0]);
    const int e = rint_u(s + 1, ve - 1, u2[1]);
    bool success = false;
    if (s < e) {
        auto t = [&](int j) -> int { return (j >= s && j <= e) ? row[s + e - j] : row[j]; };
        double old_sub = 0.0, new_sub = 0.0;
        for (int j = s; j < e; ++j) old_sub += dist32(loc, row[j], row[j + 1]);
        double old_conn = 0.0;
        old_conn += dist32(loc, row[s - 1], row[s]);
        if (e < ve - 1) old_conn += dist32(loc, row[e], row[e + 1]);
        for (int j = s; j < e; ++j) new_sub += dist32(loc, t(j), t(j + 1));
        double new_conn = 0.0;
        new_conn += dist32(loc, t(s - 1), t(s));
        if (e < ve - 1) new_conn += dist32(loc, t(e), t(e + 1));
        const double change = (new_sub + new_conn) - (old_sub + old_conn);
        if (cur + change <= safe) {
            bool dup = false;
            Bits128 seen;
            for (int j = 0; j < ve; ++j) {
                const int x = t(j);
                if (x != 0) {
                    if (seen.test(x)) { dup = true; break; }
                    seen.set(x);
                }
            }
            double total = dist32(loc, 0, t(0));
            for (int j = 1; j < ve; ++j) total += dist32(loc, t(j - 1), t(j));
            if (total <= safe && !dup) {
                reverse_row(row, s, e);
                success = true;
            }
        }
    }
    if (!success && cz >= 0) row[cz] = cz_old;
}

enum { PRIZE_PCTSP = 0, PRIZE_OP = 1 };

template <int ENV>
struct PrizeOps {
    static constexpr int ENV_FLOATS = 2 * EV_MAX;  // prize [M], aux [M]: penalty (PCTSP) / max_length (OP)
    static constexpr bool INIT_MUTATE = true;
    // PCTSP crossover: [O][2 * EV_MAX] bytes, a thread's node tables
    static constexpr size_t tail_bytes(int O) { return ENV == PRIZE_PCTSP ? (size_t)O * 2 * EV_MAX : 0; }
    const float2* loc; float* prize; float* aux; uint8_t* scratch; int L, M;
    double global_max; float pen_total, worst;
    __device__ __forceinline__ void load(const EaArgs& a, int64_t b, float* env, uint8_t* tail, const float2* loc_, int lane)
    {
        loc = loc_; prize = env; aux = env + EV_MAX; scratch = tail; L = a.L; M = a.M;
        worst = ENV == PRIZE_PCTSP ? (float)(2.5 * (double)L) : 0.0f;
        for (int i = threadIdx.x; i < M; i += EVB) {
            prize[i] = a.prize[b * M + i];
            aux[i] = a.aux[b * M + i];
        }
        global_max = (double)a.aux[b * M];                                // OP: td["max_length"][0], the depot's entry
        // penalties of all customers, lane tree over aux[1..M-1] (every wavefront computes the same value)
        pen_total = ENV == PRIZE_PCTSP ? chunked_tree_sum(M - 1, lane, [&](int t) { return a.aux[b * M + 1 + t]; }) : 0.0f;
    }
    __device__ __forceinline__ void mutate_row(int16_t* row, const double* u2) const
    {
        if (ENV == PRIZE_PCTSP) pctsp_mutate_row(row, L, u2);
        else op_mutate_row(row, L, loc, global_max, u2);
    }
    __device__ __forceinline__ void init_mutate(const EaArgs& a, int16_t* row, int64_t i) const { mutate_row(row, a.init_mut_u + i * 2); }
    __device__ __forceinline__ void mutate(const EaArgs& a, int16_t* o, int64_t dm) const { mutate_row(o, a.mut_u + dm * 2); }
    __device__ __forceinline__ bool child(const EaArgs& a, const int16_t* p1, const int16_t* p2, int role, int16_t* o,
                                          int64_t dp, int tid) const
    {
        if (ENV == PRIZE_PCTSP) {
            pctsp_child(p1, p2, role, o, L, M, prize, aux, scratch + (size_t)tid * 2 * EV_MAX);
            return false;
        }
        const int e1 = valid_end_from_one(p1, L), e2 = valid_end_from_one(p2, L);
        int max_cross = e1 - 1 < e2 - 1 ? e1 - 1 : e2 - 1;
        max_cross = max_cross < L - 1 ? max_cross : L - 1;
        if (p1[e1 - 1] != 0 || p2[e2 - 1] != 0 || max_cross <= 1) return true;
        return !op_child(role ? p2 : p1, rint_u(1, max_cross, a.cross_u[dp]), o, L, M, loc, global_max);
    }
    __device__ __forceinline__ float fitness(const int16_t* row, int lane) const
    {
        if (ENV == PRIZE_PCTSP) {
            const float len = wave_route_length(row, loc, L, lane);
            const float saved = wave_gather_sum(row, aux, L, lane);
            const float reward = saved - (len + pen_total);
            return worst - (0.0f - reward);
        }
        return worst - (0.0f - wave_gather_sum(row, prize, L, lane));
    }
};

}  // namespace

int launch_ea_prize(int env, const float* locs, const float* prize, const float* aux, int64_t* pop, float* fitness, int64_t B,
                    int S, int N, int L, int G, double mutation_rate, double crossover_rate, double selection_rate, int top_k,
                    const double* init_mut_rand, const double* init_mut_u, const double* cross_rand, const double* cross_u,
                    const double* mut_rand, const double* mut_u, hipStream_t st)
{
    EaArgs a{};
    a.locs = locs; a.prize = prize; a.aux = aux; a.pop = pop; a.fitness = fitness;
    a.B = B; a.S = S; a.N = N; a.M = N + 1; a.L = L; a.G = G; a.top_k = top_k;
    a.mutation_rate = mutation_rate; a.crossover_rate = crossover_rate;
    a.init_mut_rand = init_mut_rand; a.init_mut_u = init_mut_u; a.cross_rand = cross_rand; a.cross_u = cross_u;
    a.mut_rand = mut_rand; a.mut_u = mut_u;
    return env == EAMRL_ENV_PCTSP ? ea_launch<PrizeOps<PRIZE_PCTSP>>(a, selection_rate, st)
                                  : ea_launch<PrizeOps<PRIZE_OP>>(a, selection_rate, st);
}

}  // namespace eamrl
