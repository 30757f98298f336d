"""Vertex enumeration and the recursive-feasibility certificate on the device: device ms and vertices/s of
Solution.vertices, the largest per-region count, OVERFLOW regions and the largest intermediate list on c2x20, c3 at max_levels=4, the
complete c3 and c4 at max_levels=4 (or complete with --c4-complete), against a host loop over scipy.spatial.HalfspaceIntersection on the
same regions (this tool only), and the certificate's LP time with the c2 and c3 plants.  Writes profiles/vertex_bench.json."""
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


def _solve(name):
    import bench
    from ppopt_amd.mp_solvers import mpqp_hip_combi_graph, mpqp_hip_combinatorial
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if name in ('c2', 'c2x20'):
            return solve_mpqp(bench.build_program(name), mpqp_algorithm.combinatorial)
        if name == 'c3_l4':
            return mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4)
        if name == 'c3_graph':
            return mpqp_hip_combi_graph.solve_graph(bench.build_program('c3'))
        if name == 'c4_l4':
            return mpqp_hip_combinatorial.solve(bench.build_program('c4'), max_levels=4)
        if name == 'c4':
            return mpqp_hip_combi_graph.solve_graph(bench.build_program('c4'))
    raise KeyError(name)


def host_loop(sol, limit):
    """scipy HalfspaceIntersection from each region's Chebyshev centre, over the first `limit` regions: seconds per region"""
    import vertex_reference as ref
    ef, row_off, _ = sol._stacked()
    n = min(limit, len(row_off) - 1)
    t0 = time.perf_counter()
    nv = 0
    for i in range(n):
        f, E = ef[row_off[i]:row_off[i + 1], 0], ef[row_off[i]:row_off[i + 1], 1:]
        try:
            nv += len(ref.qhull(E, f))
        except Exception:
            pass
    dt = time.perf_counter() - t0
    return {'regions': n, 'seconds': dt, 'ms_per_region': 1e3 * dt / max(1, n), 'vertices': nv}


def main():
    from ppopt_amd import problem_generator as pg
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='c2x20,c3_l4,c3_graph,c4_l4')
    ap.add_argument('--host-limit', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vertex_bench.json'))
    args = ap.parse_args()
    out = {'cases': {}}
    plants = {'c2x20': pg.double_integrator_plant(5), 'c3_l4': pg.quad_tank_plant(), 'c3_graph': pg.quad_tank_plant()}
    for name in args.cases.split(','):
        t0 = time.perf_counter()
        sol = _solve(name)
        solve_s = time.perf_counter() - t0
        sol.vertices()                          # warm-up (module load, first allocation)
        sol._vertex_sets = None
        t0 = time.perf_counter()
        rv = sol.vertices()
        wall = time.perf_counter() - t0
        counts = numpy.diff(rv.offsets)
        rec = {'regions': len(rv), 'n_theta': int(rv.vertices.shape[1]) if rv.vertices.ndim == 2 else None, 'solve_s': solve_s,
               'device_ms': rv.stats['ms'], 'wall_s': wall, 'vertices': int(len(rv.vertices)),
               'vertices_per_s_device': len(rv.vertices) / max(1e-9, rv.stats['ms'] * 1e-3), 'max_per_region': int(counts.max()),
               'mean_per_region': float(counts.mean()), 'stats': rv.stats}
        rec['host_qhull'] = host_loop(sol, args.host_limit)
        rec['host_qhull']['vertices_per_s'] = rec['host_qhull']['vertices'] / max(1e-9, rec['host_qhull']['seconds'])
        rec['device_ms_per_region'] = rv.stats['ms'] / max(1, len(rv))
        if name in plants:
            p = plants[name]
            t0 = time.perf_counter()
            cert = sol.certify_recursive_feasibility(p['A'], p['B'], p['inputs'])
            rec['certificate'] = dict(cert.stats, wall_s=time.perf_counter() - t0, certified=cert.certified,
                                      max_margin=float(numpy.nanmax(cert.margin)) if numpy.isfinite(cert.margin).any() else None)
        out['cases'][name] = rec
        print(name, json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:          # after every case: a long one that is cut off keeps the others
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
