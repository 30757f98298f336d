"""Projections of polytopes (geometry.project): items, rows before, at the peak and after, steps, LPs, pivots per LP, device
time in sum and per LP, wall time; one run each after a warm-up call.

    python tools/project_bench.py [--out profiles/project_bench.json] [--cases seeded,copies,c3_l4]

Cases: the seeded sets of tests/project_cases.py; 10,000 copies of the first polytope of its (4, 2, 8) set in one call; the one-step
controllable sets (controllable_pre) of every region of the four-level config 3 as targets, under its plant and the input box
|u| <= 1 of the program.  No speed threshold is set; the yardstick printed beside each result is the 10.2 to 363 ns per LP of k_reduce_rows
(DESIGN §3.22), the same engine on the same kind of rows.
"""
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

YARDSTICK = 'k_reduce_rows: 10.2 to 363 ns per LP (DESIGN §3.22)'
TOL = 1e-8


def record(case, r, wall_ms, **more):
    s = r.stats
    rec = {'case': case, 'items': len(r), 'rows_before': s['rows_before'], 'rows_at_peak': int(r.peak.astype(numpy.int64).sum()),
           'max_peak': int(r.peak.max()), 'rows_after': s['rows_after'], 'steps': s['steps'], 'rows_made': s['rows_made'], 'lps': s['lps'],
           'pivots_per_lp': s['pivots'] / max(1, s['lps']), 'device_ms': s['device_ms'], 'device_ns_per_lp': 1e6 * s['device_ms'] / max(1, s['lps']),
           'wall_ms': wall_ms, 'thin': s['thin'], 'whole': s['whole'], 'too_large': s['too_large'], 'wide': s['wide'], 'yardstick': YARDSTICK}
    rec.update(more)
    print(json.dumps(rec), flush=True)
    return rec


def timed(call):
    call()                                                                     # warm pools
    t0 = time.perf_counter()
    r = call()
    return r, (time.perf_counter() - t0) * 1e3


def rows_case(name, polys, n, n_elim, out_cap=512):
    import exit_cases as ec
    from ppopt_amd.geometry import project_rows_of
    off, ef = ec.csr(polys)
    r, wall = timed(lambda: project_rows_of(off, ef, n, list(range(n - n_elim)), tol=TOL, out_cap=out_cap))
    return record(name, r, wall, n=n, n_elim=n_elim)


def seeded_cases():
    import project_cases as pc
    return [rows_case(f'seeded n={c[0]} n_elim={c[1]} tangent={c[2]}', pc.seeded_set(*c), c[0], c[1]) for c in pc.SETS + [pc.WIDE_DIM, pc.MANY_ROWS]]


def copies_case(count=10000):
    import project_cases as pc
    c = pc.SETS[3]
    return [rows_case(f'{count} copies of a polytope of n={c[0]} n_elim={c[1]} tangent={c[2]}', [pc.seeded_set(*c)[0]] * count, c[0], c[1], out_cap=64)]


def pre_case(name):
    from transition_bench import solve
    from ppopt_amd.geometry import Polytope, controllable_pre
    sol, plant = solve(name)
    n_u = numpy.asarray(plant['B']).reshape(sol.theta_dim(), -1).shape[1]
    U = Polytope(numpy.vstack([numpy.eye(n_u), -numpy.eye(n_u)]), numpy.ones((2 * n_u, 1)))
    targets = [Polytope(numpy.asarray(r.E, dtype=float), numpy.asarray(r.f, dtype=float).reshape(-1, 1)) for r in sol.critical_regions]
    targets = [t for t in targets if numpy.all(numpy.linalg.norm(t.A, axis=1) > 0.0)]
    r, wall = timed(lambda: controllable_pre(targets, plant['A'], plant['B'], U, tol=TOL, out_cap=256))
    return [record(f'controllable_pre of the regions of {name}', r, wall, n=sol.theta_dim() + n_u, n_elim=n_u, regions=len(sol))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='seeded,copies,c3_l4')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'project_bench.json'))
    args = ap.parse_args()
    out = []
    for name in args.cases.split(','):
        out.extend(seeded_cases() if name == 'seeded' else copies_case() if name == 'copies' else pre_case(name))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
