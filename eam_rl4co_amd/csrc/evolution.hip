// The LDS path of the TSP and CVRP evolutionary improvement (the fork's EA.run): k_ea of evolution_common.hpp with the
// operators of evolution_routes.hpp on Bits128 node sets -- populations of up to 128 rows of up to 128 nodes.
#include "evolution_routes.hpp"

namespace eamrl {

int launch_ea_tsp(const float* locs, int64_t* pop, float* fitness, int64_t B, int S, int N, int G, double mutation_rate,
                  double crossover_rate, double selection_rate, const double* cross_rand, const int32_t* cross_idx,
                  const double* mut_rand, const int32_t* mut_idx, hipStream_t st)
{
    EaArgs a{};
    a.locs = locs; a.pop = pop; a.fitness = fitness; a.B = B; a.S = S; a.N = N; a.M = N; a.L = N; a.G = G;
    a.mutation_rate = mutation_rate; a.crossover_rate = crossover_rate;
    a.cross_rand = cross_rand; a.cross_idx = cross_idx; a.mut_rand = mut_rand; a.mut_idx = mut_idx;
    return ea_launch<TspOps<Bits128>>(a, selection_rate, st);
}

int launch_ea_cvrp(const float* locs, const float* demand, const float* vcap, int64_t* pop, float* fitness, int64_t B, int S,
                   int N, int L, int G, double mutation_rate, double crossover_rate, double selection_rate, int top_k,
                   const double* init_mut_rand, const double* init_mut_u, const double* cross_rand, const double* cross_u,
                   const double* mut_rand, const double* mut_u, hipStream_t st)
{
    EaArgs a{};
    a.locs = locs; a.demand = demand; a.vcap = vcap; a.pop = pop; a.fitness = fitness;
    a.B = B; a.S = S; a.N = N; a.M = N + 1; a.L = L; a.G = G; a.top_k = top_k;
    a.mutation_rate = mutation_rate; a.crossover_rate = crossover_rate;
    a.init_mut_rand = init_mut_rand; a.init_mut_u = init_mut_u; a.cross_rand = cross_rand; a.cross_u = cross_u;
    a.mut_rand = mut_rand; a.mut_u = mut_u;
    return ea_launch<CvrpOps<Bits128>>(a, selection_rate, st);
}

}  // namespace eamrl
