"""Hit-and-run on the device (mpc_hit_and_run) and Solution.sample_check.  One JSON line:
  * chain steps/s of the kernel on boxes and random dense polytopes at (n, m) in SHAPES, 2^18 chains of one polytope, warmed up,
    device-event time of windows of >= 0.2 s; the fp64 rate of the operation count 2 m n FMA + m divisions per step (plus the
    Box-Muller pairs, counted as one operation each) against the 78.6 TFLOP/s vector peak; and the same chains on the vectorised
    numpy replay (tests/hit_and_run_reference.py) on this process's CPU threads, for scale;
  * sample_check wall time and coverage for bench.py's config 4 at max_levels=5, the complete config 4 (graph) and one
    mixed-integer program.

    python tools/hit_and_run_bench.py [--chains N] [--skip-check]
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
from ppopt_amd import _lib  # noqa: E402

SHAPES = [(2, 8), (8, 16), (8, 64), (10, 128), (16, 64), (33, 128), (64, 256)]
FP64_PEAK = 78.6e12


def polytope(kind, n, m, seed=0):
    rng = numpy.random.default_rng(seed)
    if kind == 'box':
        # a box of 2n rows, padded to m rows with redundant copies scaled by 2 (the kernel reads every row)
        A = numpy.vstack([numpy.eye(n), -numpy.eye(n)])
        b = numpy.ones(2 * n)
        reps = (m + 2 * n - 1) // (2 * n)
        A, b = numpy.vstack([A] * reps)[:m], numpy.concatenate([b] + [2 * b] * (reps - 1))[:m]
        return A, b
    # dense rows: a randomly rotated cube (bounded) and random unit rows; every facet at distance 1 from the origin
    Q, _ = numpy.linalg.qr(rng.standard_normal((n, n)))
    A = numpy.vstack([Q, -Q, rng.standard_normal((max(0, m - 2 * n), n))])[:m]
    A /= numpy.linalg.norm(A, axis=1, keepdims=True)
    return A, numpy.ones(m)


def kernel_rate(kind, n, m, chains):
    A, b = polytope(kind, n, m)
    off, ab, start = numpy.array([0, m]), numpy.hstack([b[:, None], A]), numpy.zeros((1, n))
    _, st = _lib.hit_and_run(off, ab, start, chains, 1, 8, 1)              # warm-up, and the chains must run
    if not (st == 0).all():
        return {'kind': kind, 'n': n, 'm': m, 'error': f'status {numpy.bincount(st.ravel()).tolist()}'}
    steps = 8
    while True:
        _lib.hit_and_run(off, ab, start, chains, 1, steps, 2)
        ms = _lib.hit_and_run.last_ms
        if ms >= 200.0 or steps >= 1 << 20:
            break
        steps = int(steps * max(2.0, 250.0 / max(ms, 1e-3)))
    runs = []
    for rep in range(3):
        _lib.hit_and_run(off, ab, start, chains, 1, steps, 3 + rep)
        runs.append(_lib.hit_and_run.last_ms)
    ms = float(numpy.median(runs))
    rate = chains * steps / (ms * 1e-3)
    ops = 2 * (2 * m * n) + m + (n + 1) // 2          # flops per step: 2 m n FMA, m divisions, the Box-Muller pairs
    return {'kind': kind, 'n': n, 'm': m, 'chains': chains, 'steps': steps, 'ms': [round(v, 3) for v in runs],
            'steps_per_s': rate, 'fp64_tflops': rate * ops / 1e12, 'share_of_fp64_peak': rate * ops / FP64_PEAK}


def numpy_rate(kind, n, m, chains=4096, steps=8):
    import hit_and_run_reference as hr
    A, b = polytope(kind, n, m)
    t = time.perf_counter()
    hr.chains(A, b, numpy.zeros(n), chains, 1, steps, 1)
    return chains * steps / (time.perf_counter() - t)


def check(sol, num_samples, per_region):
    rep = sol.sample_check(num_samples=num_samples, per_region=per_region)
    return {'regions': len(sol), 'num_samples': rep.n_samples, 'feasible': rep.n_feasible, 'uncovered': rep.n_uncovered,
            'covered_fraction': rep.covered_fraction, 'wrong': rep.n_wrong, 'spurious': rep.n_spurious, 'spurious_bad': rep.n_spurious_bad,
            'max_obj_gap': rep.max_obj_gap, 'max_x_err': rep.max_x_err, 'per_region': per_region, 'regions_sampled': rep.n_regions_sampled,
            'regions_not_sampled': rep.n_regions_not_sampled, 'failing_regions': len(rep.failing_regions), 'ok': rep.ok,
            'seconds': round(rep.seconds, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=1 << 18)
    ap.add_argument('--skip-check', action='store_true')
    args = ap.parse_args()
    out = {'tool': 'hit_and_run_bench', 'cpu_threads': os.environ.get('OMP_NUM_THREADS'), 'kernel': []}
    for kind in ('box', 'dense'):
        for n, m in SHAPES:
            if m < 2 * n:
                continue
            r = kernel_rate(kind, n, m, args.chains)
            r['numpy_steps_per_s'] = numpy_rate(kind, n, m)
            out['kernel'].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    if not args.skip_check:
        from ppopt_amd import MPQP_Program, problem_generator as pg
        from ppopt_amd.mp_solvers import mpqp_hip_combi_graph, mpqp_hip_combinatorial
        d = pg.generate_mpqp_data(20, 8, 20, 0)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            prog = MPQP_Program(d['A'], d['b'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], d['F'])
        sol = mpqp_hip_combinatorial.solve(prog, max_levels=5)
        out['c4_max_levels_5'] = check(sol, 100_000, 8)
        print(json.dumps(out['c4_max_levels_5']), file=sys.stderr, flush=True)
        gsol = mpqp_hip_combi_graph.solve_graph(prog)
        out['c4_complete_graph'] = check(gsol, 100_000, 8)
        print(json.dumps(out['c4_complete_graph']), file=sys.stderr, flush=True)
        from test_gpu_mi import _load, build
        from ppopt_amd.mp_solvers.solve_mpmiqp import solve_mpmiqp
        mi = solve_mpmiqp(build(_load('mpMIQP_market_problem')), num_cores=1)
        out['mi_mpMIQP_market_problem'] = check(mi, 100_000, 8)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
