"""The law gap (Solution.compare) on solved workloads: a solution against itself and a merged solution against its source:
regions, candidate pairs, meeting pairs, LPs and pivots, device time, pairs per second, the host sweep and the wall time.

    python tools/compare_bench.py [--out profiles/compare_bench.json] [--cases c2,c3_l4,c3]
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUTPUTS = {'c2': [10], 'c3_l4': [0, 1], 'c3': [0, 1]}      # the first input of each controller


def solve(name):
    import bench
    from ppopt_amd.mp_solvers import mpqp_hip_combinatorial, mpqp_hip_geometric
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        # the drivers directly: solve_mpqp flags what it returns overlapping, which compare refuses
        if name == 'c2':
            return mpqp_hip_combinatorial.solve(bench.build_program('c2'))
        if name == 'c3_l4':
            return mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4)
        if name == 'c3':
            return mpqp_hip_geometric.solve(bench.build_program('c3'))
    raise KeyError(name)


def record(case, kind, a, b, outputs):
    a.compare(b, outputs=outputs)      # warm pools
    t0 = time.perf_counter()
    g = a.compare(b, outputs=outputs)
    wall = time.perf_counter() - t0
    st = g.stats
    return {'case': case, 'kind': kind, 'n_theta': a.theta_dim(), 'regions_a': g.n_a, 'regions_b': g.n_b, 'outputs': g.outputs, 'wall_s': wall,
            'max_gap': g.max_gap, 'wide': g.wide, 'unmatched_a': len(g.unmatched_a), 'unmatched_b': len(g.unmatched_b), 'stats': st,
            'pairs_per_s': st['pairs'] / max(1e-9, st['pair_ms'] * 1e-3), 'pivots_per_lp': st['pivots'] / max(1, st['lps'])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='c2,c3_l4,c3')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'compare_bench.json'))
    args = ap.parse_args()
    out = []
    for name in args.cases.split(','):
        sol = solve(name)
        merged = sol.merge_regions(outputs=OUTPUTS[name])
        for rec in (record(name, 'self', sol, sol, None), record(name, 'merged_vs_source', merged, sol, OUTPUTS[name])):
            print(json.dumps(rec), flush=True)
            out.append(rec)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as fh:
                json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
