"""2-D slices of solved programs on the device (Solution.slice_2d, mpc_slice_polygons).  One JSON line:
  * per workload: the regions and their rows, the kernel time (device events, ``_lib.slice_polygons.last_ms``), the host time of
    Solution._stacked() (the [f | E] rows), and the end-to-end time of slice_2d (rows, the four box LPs, copies, kernel), as
    medians over --repeats calls after one warm-up call;
  * for scale, the scipy reference (tests/slice_reference.py) per region on a sample of 200 regions: a host reference, not a
    baseline of the device code.
Workloads: c2 (double integrator, the full combinatorial tree), the complete c3 (quad-tank, geometric) and the complete config 4
(graph, 227,349 regions) in the plane of its first two parameters, the others at the middle of the parameter box.

    python tools/slice_bench.py [--workloads c2,c3,c4] [--repeats 5] [--out profiles/slice_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from ppopt_amd import _lib  # noqa: E402


def solve(name):
    import bench
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    algo = {'c2': mpqp_algorithm.combinatorial, 'c3': mpqp_algorithm.geometric, 'c4': mpqp_algorithm.graph}[name]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        prog = bench.build_program(name)
        t0 = time.perf_counter()
        sol = solve_mpqp(prog, algo)
    return sol, time.perf_counter() - t0


def middle_of_box(sol):
    """{t: middle of the parameter set's extent in theta_t} for t >= 2 (one LP batch)."""
    P = sol.program
    n_t = sol.theta_dim()
    A, b = numpy.asarray(P.A_t, float), numpy.asarray(P.b_t, float).reshape(-1)
    C = numpy.vstack([numpy.eye(n_t), -numpy.eye(n_t)])
    st, _, obj, _ = _lib.lp_solve_batch(A, b, C, numpy.zeros((2 * n_t, len(b)), dtype=numpy.uint8))
    assert (st == _lib.LP_OPTIMAL).all()
    return {t: 0.5 * (obj[t] - obj[n_t + t]) for t in range(2, n_t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='c2,c3,c4')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'slice_bench.json'))
    args = ap.parse_args()
    import slice_reference as ref
    if _lib.load().mpc_device_count() < 1:
        raise SystemExit('slice_bench needs a GPU')
    rec = {'tool': 'tools/slice_bench.py', 'repeats': args.repeats, 'workloads': {}}
    for name in args.workloads.split(','):
        sol, solve_s = solve(name)
        fixed = middle_of_box(sol) if sol.theta_dim() > 2 else None
        sl = sol.slice_2d(fixed=fixed)                         # warm-up (code objects, pools)
        kern, stacked, e2e = [], [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            ef, row_off, _ = sol._stacked()
            stacked.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            sl = sol.slice_2d(fixed=fixed, box=sl.box)      # the box of the warm-up: end to end without the four LPs ...
            e2e.append(1e3 * (time.perf_counter() - t0))
            kern.append(_lib.slice_polygons.last_ms)
        t0 = time.perf_counter()
        sol.slice_2d(fixed=fixed)                              # ... and once with them
        e2e_lp = 1e3 * (time.perf_counter() - t0)
        rng = numpy.random.default_rng(0)
        sample = rng.choice(len(sol.critical_regions), size=min(200, len(sol.critical_regions)), replace=False)
        t0 = time.perf_counter()
        for r in sample:
            cr = sol.critical_regions[int(r)]
            ref.slice_polygon(numpy.asarray(cr.E, float), numpy.asarray(cr.f, float).reshape(-1), sl.theta_0, sl.U, sl.box)
        ref_ms = 1e3 * (time.perf_counter() - t0) / len(sample)
        rec['workloads'][name] = {
            'regions': len(sol.critical_regions), 'rows': int(row_off[-1]), 'n_theta': sol.theta_dim(), 'solve_s': round(solve_s, 2),
            'box': [float(v) for v in sl.box], 'full_polygons': int(numpy.count_nonzero(sl.full())),
            'area_sum': float(numpy.sum(sl.areas[sl.full()])),
            'kernel_ms': statistics.median(kern), 'kernel_ms_all': kern, 'stacked_ms': statistics.median(stacked),
            'slice_2d_ms': statistics.median(e2e), 'slice_2d_with_box_lps_ms': e2e_lp,
            'host_reference_ms_per_region': ref_ms, 'host_reference_sample': int(len(sample))}
        print(name, json.dumps(rec['workloads'][name]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(rec, fh)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
