"""Search-tree build and query rates on the device: for every case the build stages, the classification work, the tree's
shape, and location rates of the tree against the scan (and the walk where it applies) at 1e5 and 1e6 points.

    python tools/tree_bench.py [--out profiles/tree_bench.json] [--cases c2x20,c3_l4,c3_graph,c4_l5,mi_market]
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
    from ppopt_amd.mp_solvers import mpqp_hip_combinatorial
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if name == 'c2x20':
            return solve_mpqp(bench.build_program('c2x20'), mpqp_algorithm.combinatorial)
        if name == 'c3_l4':
            return mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4)
        if name == 'c3_graph':
            return solve_mpqp(bench.build_program('c3'), mpqp_algorithm.graph)
        if name == 'c4_l5':
            return mpqp_hip_combinatorial.solve(bench.build_program('c4'), max_levels=5)
        if name == 'mi_market':
            from test_export import mixed_integer_solution
            return mixed_integer_solution('mpMIQP_market_problem')[0]
    raise KeyError(name)


def rate(fn, pts, reps=3):
    fn(pts)
    best = float('inf')
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(pts)
        best = min(best, time.perf_counter() - t0)
    return len(pts) / best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='c2x20,c3_l4,c3_graph,c4_l5,mi_market')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tree_bench.json'))
    ap.add_argument('--sizes', default='100000,1000000')
    args = ap.parse_args()
    from ppopt_amd import _lib
    from ppopt_amd.upop import SearchTree
    from ppopt_amd.upop.linear_code_gen import plane_table
    out = []
    for name in args.cases.split(','):
        sol = solve(name)
        t0 = time.perf_counter()
        try:
            tree = SearchTree.build(sol)
        except _lib.MpcError as e:   # a refused or degenerate build is a result too
            rec = {'case': name, 'regions': len(sol), 'n_theta': sol.theta_dim(),
                   'planes': int(len(plane_table(sol.critical_regions, sol.theta_dim())[0])), 'build_error': str(e),
                   'build_wall_s': time.perf_counter() - t0}
            print(json.dumps(rec), flush=True)
            out.append(rec)
            continue
        wall = time.perf_counter() - t0
        leaf = tree.leaf_sizes()
        rec = {'case': name, 'regions': len(sol), 'n_theta': sol.theta_dim(), 'planes': int(len(tree.planes)), 'build_wall_s': wall,
               'stats': tree.stats, 'depth': tree.depth(), 'nodes': tree.n_nodes, 'leaves': int(len(leaf)),
               'leaf_max': int(leaf.max()) if len(leaf) else 0, 'leaf_mean': float(leaf.mean()) if len(leaf) else 0.0, 'rates': {}}
        ef, row_off, _ = sol._stacked()
        rng = numpy.random.default_rng(0)
        centre, _, status = _lib.facet_centres(ef, row_off)
        ok = centre[(status == 0) & numpy.all(numpy.isfinite(centre), axis=1)]
        lo, hi = ok.min(axis=0), ok.max(axis=0)
        loc = sol.locator()
        for m in (int(v) for v in args.sizes.split(',')):
            pts = rng.uniform(lo, hi, size=(m, sol.theta_dim()))
            r = {'tree_pts_per_s': rate(tree.locate_batch, pts)}
            if m <= 100_000 or len(sol) <= 10_000:
                r['scan_pts_per_s'] = rate(lambda p: loc.query(p, sol.point_location_tolerance, sol.is_overlapping, want_x=False), pts,
                                           reps=1 if m > 100_000 else 3)
            if loc.has_adjacency and not sol.is_overlapping:
                r['walk_pts_per_s'] = rate(lambda p: loc.query(p, sol.point_location_tolerance, False, want_x=False, walk=True), pts)
            assert numpy.array_equal(tree.locate_batch(pts), sol.get_region_batch(pts)), name
            rec['rates'][str(m)] = r
        print(json.dumps(rec), flush=True)
        out.append(rec)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
