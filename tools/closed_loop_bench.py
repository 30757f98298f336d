"""Closed-loop simulation (Solution.simulate) on solved MPC workloads: trajectory-steps/s of the fused kernel for every
locator, device ms, walk crossings per step and fallbacks, against the per-step loop over evaluate_batch (same arithmetic, checked to give
the same final states) and the host reference loop on a small sample.

    python tools/closed_loop_bench.py [--out profiles/closed_loop_bench.json] [--cases c2x20,c3_l4,c3_graph] [--sizes 100000,1000000]
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
    from ppopt_amd.mp_solvers import mpqp_hip_combi_graph, mpqp_hip_combinatorial
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if name == 'c2x20':
            return solve_mpqp(bench.build_program('c2x20'), mpqp_algorithm.combinatorial)
        if name == 'c3_l4':
            return mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4)
        if name == 'c3_graph':
            return mpqp_hip_combi_graph.solve_graph(bench.build_program('c3'))
    raise KeyError(name)


def plant(name):
    from ppopt_amd import problem_generator as pg
    return pg.double_integrator_plant(5) if name.startswith('c2') else pg.quad_tank_plant()


def starts(sol, n, seed):
    """uniform over the box of the regions' facet centres, widened by 20 % on every side"""
    from ppopt_amd import _lib
    ef, row_off, _ = sol._stacked()
    centre, _, status = _lib.facet_centres(ef, row_off)
    c = centre[(status == 0) & numpy.all(numpy.isfinite(centre), axis=1)]
    lo, hi = c.min(axis=0), c.max(axis=0)
    span = numpy.maximum(hi - lo, 1e-3)
    return numpy.random.default_rng(seed).uniform(lo - 0.2 * span, hi + 0.2 * span, size=(n, ef.shape[1] - 1))


def step_loop(sol, th0, steps, pl):
    """the user's loop: evaluate_batch every step (copies and a synchronisation each), the device's plant arithmetic on the host"""
    from ppopt_amd.closed_loop import replay_step
    th = th0.copy()
    live = numpy.arange(len(th))
    for _ in range(steps):
        x, r = sol.evaluate_batch(th[live])
        ok = r >= 0
        live = live[ok]
        if not len(live):
            break
        th[live] = replay_step(th[live], x[ok][:, pl['inputs']], pl['A'], pl['B'])
    return th


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='c2x20,c3_l4,c3_graph')
    ap.add_argument('--sizes', default='100000,1000000')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--host-sample', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'closed_loop_bench.json'))
    args = ap.parse_args()
    import closed_loop_reference as ref
    out = []
    K = args.steps
    for name in args.cases.split(','):
        sol = solve(name)
        pl = plant(name)
        modes = ['scan', 'tree'] + (['walk'] if sol.is_complete and not sol.is_overlapping else [])
        t0 = time.perf_counter()
        sol.search_tree()
        tree_s = time.perf_counter() - t0
        for n in (int(v) for v in args.sizes.split(',')):
            th0 = starts(sol, n, 1)
            rec = {'case': name, 'regions': len(sol), 'n': n, 'steps': K, 'tree_build_s': tree_s, 'modes': {}}
            final = None
            for m in modes:
                sol.simulate(th0[:1024], K, pl['A'], pl['B'], pl['inputs'], locate=m, record='final')        # warm-up
                t0 = time.perf_counter()
                res = sol.simulate(th0, K, pl['A'], pl['B'], pl['inputs'], locate=m, record='final')
                wall = time.perf_counter() - t0
                st = res.stats
                rec['modes'][m] = {'device_ms': st['ms'], 'wall_s': wall, 'trajectory_steps': st['trajectory_steps'],
                                   'steps_per_s_device': st['trajectory_steps'] / (st['ms'] * 1e-3) if st['ms'] > 0 else None,
                                   'steps_per_s_wall': st['trajectory_steps'] / wall, 'crossings_per_step': st['crossings_per_step'],
                                   'fallbacks': st['fallbacks'], 'status_counts': st['status_counts']}
                if final is None:
                    final = res
                else:
                    rec['modes'][m]['same_as_' + modes[0]] = bool(numpy.array_equal(res.theta.view(numpy.uint64), final.theta.view(numpy.uint64)))
                print(json.dumps({'case': name, 'n': n, 'mode': m, **rec['modes'][m]}), flush=True)
            # the per-step evaluate_batch loop: same final states
            t0 = time.perf_counter()
            th = step_loop(sol, th0, K, pl)
            loop_s = time.perf_counter() - t0
            live = final.status == 0
            rec['step_loop'] = {'wall_s': loop_s, 'trajectory_steps': final.stats['trajectory_steps'],
                                'steps_per_s': final.stats['trajectory_steps'] / loop_s,
                                'same_final_states': bool(numpy.array_equal(th[live], final.theta[live]))}
            print(json.dumps({'case': name, 'n': n, 'step_loop': rec['step_loop']}), flush=True)
            out.append(rec)
        # the host reference loop on a small sample
        th0 = starts(sol, args.host_sample, 2)
        sol.materialize()
        t0 = time.perf_counter()
        h = ref.simulate(sol, th0, K, pl['A'], pl['B'], pl['inputs'])
        host_s = time.perf_counter() - t0
        hs = int(numpy.sum(h['exit_step']) + numpy.sum(h['status'] == 2))
        out.append({'case': name, 'host_reference': {'n': args.host_sample, 'steps': K, 'wall_s': host_s, 'trajectory_steps': hs,
                                                     'steps_per_s': hs / host_s}})
        print(json.dumps(out[-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
