"""Second moments of regions on the device: device ms of Solution.moments beside Solution.volumes in the same process
(median of --repeats calls after a warm-up), regions, simplices and statuses on c2, c3 at max_levels=4, the complete c3 and c4 at
max_levels=4 with the default work cap, and Solution.expected_values of each.  Writes profiles/moments_bench.json."""
import argparse
import json
import os
import sys
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    from vertex_bench import _solve
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='c2,c3_l4,c3_graph,c4_l4')
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'moments_bench.json'))
    args = ap.parse_args()
    out = {'repeats': args.repeats, 'cases': {}}
    for name in args.cases.split(','):
        if name == 'c2':     # not through solve_mpqp, which flags every solution as overlapping (expected_values refuses those)
            import bench
            from ppopt_amd.mp_solvers import mpqp_hip_combinatorial
            sol = mpqp_hip_combinatorial.solve(bench.build_program('c2'))
        else:
            sol = _solve(name)
        sol.volumes(), sol.moments()                        # warm-up (module load, first allocation, the vertex pass)
        ms_v, ms_m = [], []
        for _ in range(args.repeats):                       # interleaved: both passes see the same clocks
            ms_v.append(sol.volumes().stats['ms'])
            mom = sol.moments()
            ms_m.append(mom.stats['ms'])
        t0 = time.perf_counter()
        ev = sol.expected_values()
        wall = time.perf_counter() - t0
        v, m = float(numpy.median(ms_v)), float(numpy.median(ms_m))
        rec = {'regions': len(mom), 'n_theta': int(mom.centroid.shape[1]), 'volume_pass_ms': v, 'moments_pass_ms': m, 'ratio': m / v,
               'volume_pass_ms_all': ms_v, 'moments_pass_ms_all': ms_m, 'simplices': mom.stats['simplices'],
               'max_simplices_per_region': mom.stats['max_simplices'], 'status_counts': mom.stats['status_counts'],
               'launches': mom.stats['launches'], 'expected_values_wall_s': wall,
               'expected_values': {'total': ev.total, 'objective_integral': ev.objective_integral, 'objective_mean': ev.objective_mean,
                                   'x_mean': ev.x_mean.tolist(), 'x_cov_diagonal': numpy.diag(ev.x_cov).tolist(),
                                   'theta_mean': ev.theta_mean.tolist(), 'theta_cov_diagonal': numpy.diag(ev.theta_cov).tolist(),
                                   'status_counts': ev.status_counts, 'ok': ev.ok}}
        out['cases'][name] = rec
        print(name, json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:          # after every case: a long one that is cut off keeps the others
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
