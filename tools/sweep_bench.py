"""The candidate sweep and the row screen (geometry.box_pairs) on solved workloads: Solution.transition_graph and the
self-comparison Solution.compare in four settings each -- host sweep (the behaviour without the new arguments, the baseline), device
sweep, device sweep with the row screen, host sweep with the row screen.  One warm-up call, then one timed call per record: box tests,
box candidates, the share screened out, edges or meeting pairs, the sweep's wall time (copies included), the kernel times of k_box_pairs
and k_pair_screen, the pair stage's device time, the wall time, and whether the result equals the host sweep's.

    python tools/sweep_bench.py [--out profiles/sweep_bench.json] [--cases c3_l4,c3]
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

SETTINGS = (('host', 'none'), ('device', 'none'), ('device', 'rows'), ('host', 'rows'))


def solve(name):
    import bench
    from ppopt_amd import problem_generator as pg
    from ppopt_amd.mp_solvers import mpqp_hip_combinatorial, mpqp_hip_geometric
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        # the drivers directly: solve_mpqp flags what it returns overlapping, which both calls refuse
        if name == 'c3_l4':
            return mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4), pg.quad_tank_plant()
        if name == 'c3':
            return mpqp_hip_geometric.solve(bench.build_program('c3')), pg.quad_tank_plant()
    raise KeyError(name)


def timed(call):
    call()      # warm pools
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def common(case, call, sweep, screen, st, wall_ms, found, same):
    box = st.get('box_candidates', st['candidates'])
    return {'case': case, 'call': call, 'sweep': sweep, 'screen': screen, 'box_candidates': box, 'candidates': st['candidates'],
            'screened': st.get('screened', 0), 'screened_share': st.get('screened', 0) / max(1, box), 'found': found,
            'sweep_ms': st['sweep_ms'], 'box_pairs_kernel_ms': st.get('sweep_kernel_ms'), 'screen_ms': st.get('screen_ms'),
            'pair_screen_kernel_ms': st.get('screen_kernel_ms'), 'pair_ms': st['pair_ms'], 'wall_ms': wall_ms, 'same_as_host': same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='c3_l4,c3')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sweep_bench.json'))
    args = ap.parse_args()
    out = []

    def keep(rec):
        print(json.dumps(rec), flush=True)
        out.append(rec)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)

    for name in args.cases.split(','):
        sol, plant = solve(name)
        usable = None
        base = None
        for sweep, screen in SETTINGS:
            g, wall = timed(lambda: sol.transition_graph(plant['A'], plant['B'], plant['inputs'], sweep=sweep, screen=screen))
            base = g if base is None else base
            same = all(getattr(g, k).tobytes() == getattr(base, k).tobytes() for k in ('indptr', 'indices', 'radius', 'status', 'witness'))
            rec = common(name, 'transition_graph', sweep, screen, g.stats, wall, g.stats['edges'], same)
            keep(dict(rec, regions=len(sol), n_theta=sol.theta_dim()))
        base = None
        for sweep, screen in SETTINGS:
            g, wall = timed(lambda: sol.compare(sol, sweep=sweep, screen=screen))
            base = g if base is None else base
            usable = int(g.usable_a.sum())
            m, mb = g.meets, base.meets
            same = (g.max_gap == base.max_gap and numpy.array_equal(g.i[m], base.i[mb]) and numpy.array_equal(g.j[m], base.j[mb])
                    and g.gap[m].tobytes() == base.gap[mb].tobytes() and g.radius[m].tobytes() == base.radius[mb].tobytes())
            rec = common(name, 'compare_self', sweep, screen, g.stats, wall, g.stats['meets'], bool(same))
            keep(dict(rec, regions=len(sol), n_theta=sol.theta_dim(), box_tests=g.stats['box_pairs'], usable=usable))


if __name__ == '__main__':
    main()
