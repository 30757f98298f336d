"""Region merging (Solution.merge_regions) on solved workloads: regions, planes, search-tree nodes and exported C++ size
before and after, and the merge's own work and times.

    python tools/merge_bench.py [--out profiles/merge_bench.json] [--cases c2x20,c3_l4,c3_graph,c4_l5]
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

OUTPUTS = {'c2x20': [10], 'c3_l4': [0, 1], 'c3_graph': [0, 1], 'c4_l5': [0]}


def solve(name):
    import bench
    from ppopt_amd.mp_solvers import mpqp_hip_combi_graph, mpqp_hip_combinatorial
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if name == 'c2x20':
            return solve_mpqp(bench.build_program('c2x20'), mpqp_algorithm.combinatorial)
        if name == 'c3_l4':
            return mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4)
        if name == 'c3_graph':
            # the driver directly: solve_mpqp flags the complete c3 overlapping (Q not positive definite), which merge_regions refuses
            return mpqp_hip_combi_graph.solve_graph(bench.build_program('c3'))
        if name == 'c4_l5':
            return mpqp_hip_combinatorial.solve(bench.build_program('c4'), max_levels=5)
    raise KeyError(name)


def shape(sol, tree: bool = True):
    """planes of the export, search-tree nodes (or the library's refusal) and the size of the exported C++"""
    from ppopt_amd import _lib
    from ppopt_amd.upop import SearchTree
    from ppopt_amd.upop.linear_code_gen import generate_code_cpp, plane_table
    rec = {'regions': len(sol), 'planes': int(len(plane_table(sol.critical_regions, sol.theta_dim())[0])),
           'cpp_bytes': len(generate_code_cpp(sol, float_type='double'))}
    if not tree:
        rec['tree_error'] = 'not built (refused after 76 s in profiles/tree_bench.json: a degenerate tree, DESIGN §3.13)'
        return rec
    t0 = time.perf_counter()
    try:
        tree = SearchTree.build(sol)
        rec['tree_nodes'] = int(tree.n_nodes)
        rec['tree_depth'] = int(tree.depth())
    except _lib.MpcError as e:
        rec['tree_error'] = str(e)
    rec['tree_wall_s'] = time.perf_counter() - t0
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='c2x20,c3_l4,c3_graph,c4_l5')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'merge_bench.json'))
    args = ap.parse_args()
    out = []
    for name in args.cases.split(','):
        sol = solve(name)
        outputs = OUTPUTS[name]
        t0 = time.perf_counter()
        try:
            merged = sol.merge_regions(outputs=outputs)
        except ValueError as e:      # a refused source is a result too (c2x20: Q only semidefinite, flagged overlapping)
            rec = {'case': name, 'regions': len(sol), 'overlapping': bool(sol.is_overlapping), 'refused': str(e)}
            print(json.dumps(rec), flush=True)
            out.append(rec)
            continue
        wall = time.perf_counter() - t0
        st = dict(merged.merge_info['stats'])
        rec = {'case': name, 'n_theta': sol.theta_dim(), 'outputs': outputs, 'merge_wall_s': wall, 'stats': st,
               'box_share': st['box_pairs'] / st['pairs'] if st['pairs'] else None,
               'largest_member_list': max(len(r.members) for r in merged.critical_regions) if len(merged) else 0,
               'before': shape(sol, tree=name != 'c4_l5'), 'after': shape(merged, tree=name != 'c4_l5')}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
