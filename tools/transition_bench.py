"""The transition graph (Solution.transition_graph) on solved workloads: regions, candidates, edges, LPs and pivots, device
times of the box and pair stages, the host sweep, and the CPU reference's time per pair on a sample of the candidates.

    python tools/transition_bench.py [--out profiles/transition_bench.json] [--cases c2,c3_l4,c3] [--sample 200]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def solve(name):
    import bench
    from ppopt_amd import problem_generator as pg
    from ppopt_amd.mp_solvers import mpqp_hip_combinatorial, mpqp_hip_geometric
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        # the drivers directly: solve_mpqp flags what it returns overlapping, which transition_graph refuses
        if name == 'c2':
            return mpqp_hip_combinatorial.solve(bench.build_program('c2')), pg.double_integrator_plant(5)
        if name == 'c3_l4':
            return mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4), pg.quad_tank_plant()
        if name == 'c3':
            return mpqp_hip_geometric.solve(bench.build_program('c3')), pg.quad_tank_plant()
    raise KeyError(name)


def reference_ms_per_pair(sol, plant, graph, sample: int):
    """the CPU reference (tests/transition_reference.py, HiGHS) on a seeded sample of the graph's edges and as many other pairs"""
    import transition_reference as ref
    from ppopt_amd import invariance
    from ppopt_amd.region_merge import unit_rows
    n_t = sol.theta_dim()
    polys = [unit_rows(r.E, r.f, n_t)[0] for r in sol.critical_regions]
    _, _, xlaw = sol._stacked()
    Phi, phi = invariance.closed_loop_maps(xlaw, numpy.asarray(plant['A'], dtype=float), numpy.asarray(plant['B'], dtype=float).reshape(n_t, -1),
                                           numpy.asarray(plant['inputs']))
    rng = numpy.random.default_rng(0)
    src, dst = graph.sources(), graph.indices
    pick = rng.choice(len(src), min(sample, len(src)), replace=False)
    pairs = [(int(src[k]), int(dst[k])) for k in pick] + [(int(i), int(j)) for i, j in rng.integers(0, len(polys), size=(sample, 2))]
    t0 = time.perf_counter()
    want = ref.graph_reference(polys, Phi, phi, 1e-8, pairs)
    ms = (time.perf_counter() - t0) * 1e3 / len(pairs)
    wrong = sum((v[0] != ref.NO_EDGE) != graph.has_edge(*pair) for pair, v in want.items() if not v[2])
    return ms, len(pairs), wrong


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='c2,c3_l4,c3')
    ap.add_argument('--sample', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transition_bench.json'))
    args = ap.parse_args()
    out = []
    for name in args.cases.split(','):
        sol, plant = solve(name)
        sol.transition_graph(plant['A'], plant['B'], plant['inputs'])      # warm pools
        t0 = time.perf_counter()
        g = sol.transition_graph(plant['A'], plant['B'], plant['inputs'])
        wall = time.perf_counter() - t0
        st = g.stats
        ref_ms, ref_pairs, wrong = reference_ms_per_pair(sol, plant, g, args.sample)
        rec = {'case': name, 'n_theta': sol.theta_dim(), 'regions': len(sol), 'wall_s': wall, 'stats': st,
               'pivots_per_lp': st['pivots'] / max(1, st['lps']), 'device_us_per_lp': 1e3 * st['pair_ms'] / max(1, st['lps']),
               'undecided_edges': int(numpy.sum(g.status == 3)), 'undecided_regions': int(numpy.sum(g.region_status == 3)),
               'unbounded_edges': int(numpy.sum(g.status == 2)),
               'reference_ms_per_pair': ref_ms, 'reference_pairs': ref_pairs, 'reference_disagreements': wrong}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
