#!/usr/bin/env python3
"""Golden vectors of the fork's EA.run (rl4co/models/zoo/earl/evolution.py) at shapes beyond the LDS kernel's limits -- more
than 128 TSP nodes, more than 127 CVRP customers -- produced by RUNNING THE REFERENCE exactly as make_golden_ea.py does
(its `tsp_case` / `cvrp_case`: `_refshim.install_numba()`, the recorded `np.random` draws in the structured form the
kernels take, the float64 work-array proxy for numba's typing):

    python tests/golden/make_golden_ea_large.py

The populations are small (12 tours, 3 generations) because the reference's operators run as plain Python here; the graphs
are what matters: a third 64-bit word in the node sets, TSP rows longer than 128, CVRP customers above 127 (the rows of
random feasible tours stay near N + the number of routes, 144-145 entries here; rows beyond 256 come from rollouts in the
oracle tests).
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden_ea import cvrp_case, tsp_case  # noqa: E402  (installs the shims on import)


def main():
    tsp_case("ea_large_tsp130_busy", N=130, B=2, S=12, G=3, mutation_rate=0.5, crossover_rate=0.8, selection_rate=0.5, seed=21)
    cvrp_case("ea_large_cvrp129_busy", N=129, B=2, S=12, G=3, mutation_rate=0.5, crossover_rate=0.8, selection_rate=0.5,
              seed=22)
    cvrp_case("ea_large_cvrp129_am", N=129, B=2, S=12, G=3, mutation_rate=0.5, crossover_rate=0.8, selection_rate=0.5, seed=23,
              method="am")


if __name__ == "__main__":
    main()
