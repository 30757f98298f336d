"""Region volumes on the device: regions, simplices, the largest simplex count of one region, TOO_LARGE regions and device
ms of Solution.volumes on c2x20, c3 at max_levels=4, the complete c3 and c4 at max_levels=4, the exact coverage where the solution is not
overlapping, and a host loop of scipy.spatial.ConvexHull(V).volume over the first regions (this tool only).  Writes
profiles/volume_bench.json."""
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


def host_loop(vols, limit):
    """scipy ConvexHull(V).volume over the first `limit` OK regions: seconds per region; regions qhull rejects are counted and named"""
    from scipy.spatial import ConvexHull, QhullError
    done, worst, failed = 0, 0.0, []
    t0 = time.perf_counter()
    for i in numpy.flatnonzero(vols.status == 0)[:limit]:
        try:
            v = ConvexHull(vols.vertices.of(i)).volume
        except QhullError:
            failed.append(int(i))
            continue
        worst = max(worst, abs(v - vols.volume[i]) / v)
        done += 1
    dt = time.perf_counter() - t0
    return {'regions': done, 'qhull_failed': failed, 'seconds': dt, 'ms_per_region': 1e3 * dt / max(1, done + len(failed)),
            'largest_relative_difference': worst}


def main():
    from vertex_bench import _solve
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='c2x20,c3_l4,c3_graph,c4_l4')
    ap.add_argument('--host-limit', type=int, default=30)
    ap.add_argument('--max-simplices', type=int, default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'volume_bench.json'))
    args = ap.parse_args()
    out = {'cases': {}}
    for name in args.cases.split(','):
        sol = _solve(name)
        sol.volumes(max_simplices=args.max_simplices)      # warm-up (module load, first allocation, the vertex pass)
        t0 = time.perf_counter()
        vols = sol.volumes(max_simplices=args.max_simplices)
        wall = time.perf_counter() - t0
        ok = vols.status == 0
        rec = {'regions': len(vols), 'n_theta': int(vols.centroid.shape[1]), 'device_ms': vols.stats['ms'], 'wall_s': wall,
               'simplices': vols.stats['simplices'], 'max_simplices_per_region': vols.stats['max_simplices'],
               'too_large': vols.stats['status_counts'][5], 'inconsistent': vols.stats['status_counts'][6],
               'status_counts': vols.stats['status_counts'], 'launches': vols.stats['launches'],
               'max_vertices_per_region': int(numpy.diff(vols.vertices.offsets).max()),
               'vertex_pass_ms': vols.vertices.stats['ms'], 'volume_of_ok_regions': float(vols.volume[ok].sum()),
               'device_ms_per_region': vols.stats['ms'] / max(1, len(vols)),
               'simplices_per_s_device': vols.stats['simplices'] / max(1e-9, vols.stats['ms'] * 1e-3)}
        rec['host_qhull'] = host_loop(vols, args.host_limit)
        if not sol.is_overlapping and args.max_simplices is None:
            cov = sol.coverage_volume()
            rec['coverage'] = {'total': cov.total, 'theta_volume': cov.theta_volume, 'fraction': cov.fraction, 'ok': cov.ok}
        out['cases'][name] = rec
        print(name, json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:          # after every case: a long one that is cut off keeps the others
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
