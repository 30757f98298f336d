"""The mixed-integer QP at 1e5 parameter points (MPMIQP_Program.solve_theta_batch, mpc_miqp_solve_batch): points/s and
(point, fixation) pairs/s of the device call, and the same answers the slow way -- per feasible fixation the substituted
program's QP batch (MPQP_Program.solve_theta_batch's device path), then a host argmin (first fixation on ties).  One JSON line.

    python tools/miqp_theta_bench.py [--points N]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppopt_amd import MPMIQP_Program, _lib  # noqa: E402
from ppopt_amd.problem_generator import generate_mpmiqp_data  # noqa: E402


def workload(name):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if name == 'mi_rand_6_3_12_b5_s0':
            g = numpy.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', name + '.npz'))
            return MPMIQP_Program(g['raw_A'], g['raw_b'], g['raw_c'], g['raw_H'], g['raw_Q'], g['raw_A_t'], g['raw_b_t'], g['raw_F'],
                                  g['raw_binary_indices'].tolist())
        d = generate_mpmiqp_data(10, 5, 24, 8, 0)
        return MPMIQP_Program(d['A'], d['b'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], d['F'], d['binary_indices'])


def theta_box(prog):
    nt = prog.num_t()
    lo, hi = numpy.zeros(nt), numpy.zeros(nt)
    for j in range(nt):
        for sign, out in ((1.0, lo), (-1.0, hi)):
            c = numpy.zeros((nt, 1))
            c[j, 0] = sign
            out[j] = sign * prog.solver.solve_lp(c, prog.A_t, prog.b_t).obj
    return lo, hi


def device_call(prog, B, Y, th):
    step = max(1, int(prog.solver.MILP_BATCH_BYTES // (12 * len(Y))))
    out = [_lib.miqp_solve_batch(B, Y, th[lo:lo + step]) for lo in range(0, len(th), step)]
    return numpy.concatenate([o[0] for o in out]), numpy.concatenate([o[2] for o in out])


def slow_way(prog, leaves, th):
    """Per fixation: the substituted program's QP batch on the device; objective with the substituted constants; host argmin."""
    best = numpy.full(len(th), numpy.inf)
    for y in leaves:
        sub = prog.generate_substituted_problem(y, deferred=True)
        st, x, _, _ = sub.engine().qp_solve_batch(th)
        ok = (st == 0) & numpy.all(th @ sub.A_t.T <= sub.b_t.reshape(1, -1), axis=1)
        c = sub.c.reshape(1, -1) + th @ sub.H.T
        obj = 0.5 * numpy.einsum('pi,ij,pj->p', x, sub.Q, x) + numpy.einsum('pi,pi->p', c, x) + float(sub.c_c[0, 0]) \
            + th @ sub.c_t.ravel() + 0.5 * numpy.einsum('pi,ij,pj->p', th, sub.Q_t, th)
        better = ok & (obj < best)
        best[better] = obj[better]
        sub.release_engine()
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=100000)
    args = ap.parse_args()
    rec = {'tool': 'miqp_theta_bench', 'points': args.points, 'workloads': {}}
    for name in ('mi_rand_6_3_12_b5_s0', 'gen_mpmiqp_10_5_24_b8_s0'):
        prog = workload(name)
        B = prog.theta_blocks()
        leaves = prog.feasible_combinations()
        Y = numpy.asarray(leaves, dtype=numpy.float64)
        lo, hi = theta_box(prog)
        th = numpy.random.default_rng(0).uniform(lo, hi, (args.points, prog.num_t()))
        device_call(prog, B, Y, th[:2000])            # warm-up: module load, pooled blocks
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            status, obj = device_call(prog, B, Y, th)
            times.append(time.perf_counter() - t0)
        dt = min(times)
        t0 = time.perf_counter()
        slow = slow_way(prog, leaves, th)
        dt_slow = time.perf_counter() - t0
        fast = numpy.where(status == 0, obj, numpy.inf)
        both = numpy.isfinite(fast) & numpy.isfinite(slow)
        diff = numpy.abs(fast[both] - slow[both]) / numpy.maximum(1.0, numpy.abs(slow[both]))
        rec['workloads'][name] = {
            'leaves': len(leaves), 'lcp_rows': int(B['n_c']), 'lcp_equalities': int(B['n_eq']), 'check_rows': int(B['check'].shape[0]),
            'seconds': dt, 'points_per_s': args.points / dt, 'pairs_per_s': args.points * len(leaves) / dt,
            'optimal_points': int((status == 0).sum()), 'slow_seconds': dt_slow,
            'feasibility_disagreements': int((numpy.isfinite(fast) != numpy.isfinite(slow)).sum()),
            'max_rel_obj_diff': float(diff.max()) if diff.size else None}
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
