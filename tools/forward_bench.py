"""The forward cells (Solution.reach_cells) on solved workloads, against the host-driven composition of the calls the package
had before: per step the next maps in numpy, transition_pairs on parents + regions for the item statuses, exit_sets.pulled_back_rows on
the host, and reduce_rows_of for the kept rows.  Both start from the same transition graph and the same step 0 (the regions themselves),
run in the same process after one warm-up call each, alternating, and the medians of the wall times are recorded with items, LPs, pivots
per LP, cells per step, device ms per step and device ns per LP.  Every case runs under its own plant and under a mismatched one, the
model's A scaled by 1.1 (tools/invariant_bench.py has no mismatched plant to share).

    python tools/forward_bench.py [--out profiles/forward_bench.json] [--cases c2,c3_l4,c3] [--repeats 5] [--steps 4]
"""
import argparse
import json
import os
import sys
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

MISMATCH = 1.1


def composition(off, ef, Phi, phi, n_t, succ, cells0, points0, tol, steps):
    """the iteration driven from the host: (cells per step, seconds in transition_pairs, in the host's maps and pull-back, in reduce_rows_of)"""
    from ppopt_amd import exit_sets as ex, transition as tr
    from ppopt_amd.geometry.reduce import reduce_rows_of
    polys = numpy.split(ef, off[1:-1])
    R = len(polys)
    cells = [(i, polys[i], numpy.eye(n_t), numpy.zeros(n_t), points0[n]) for n, i in enumerate(cells0)]      # region, rows, G, g, point
    per_step, t_pairs, t_back, t_reduce = [len(cells)], 0.0, 0.0, 0.0
    for _ in range(steps):
        t0 = time.perf_counter()
        nxt = [(Phi[i] @ G, Phi[i] @ g + phi[i]) for i, _, G, g, _ in cells]
        pa = [n for n, c in enumerate(cells) for _ in succ[c[0]]]
        pb = [len(cells) + int(j) for c in cells for j in succ[c[0]]]
        if not pa:
            break
        ends = numpy.cumsum([len(c[1]) for c in cells])
        aoff = numpy.concatenate([[0], ends, ends[-1] + off[1:]]).astype(numpy.int64)
        aef = numpy.vstack([c[1] for c in cells] + [ef])
        P = numpy.concatenate([numpy.asarray([m[0] for m in nxt]), numpy.tile(numpy.eye(n_t), (R, 1, 1))])
        p = numpy.concatenate([numpy.asarray([m[1] for m in nxt]), numpy.zeros((R, n_t))])
        t1 = time.perf_counter()
        res = tr.transition_pairs(aoff, aef, P, p, n_t, tol=tol, pairs=(pa, pb))
        t2 = time.perf_counter()
        edge = numpy.flatnonzero(res['status'] != tr.NO_EDGE)          # sorted by (parent, region) already
        if not len(edge):
            t_back, t_pairs = t_back + t1 - t0, t_pairs + t2 - t1
            break
        rows = []
        for e in edge:
            q, j = int(res['i'][e]), int(res['j'][e]) - len(cells)
            back = ex.pulled_back_rows(polys[j], nxt[q][0], nxt[q][1])
            rows.append(numpy.vstack([cells[q][1], back[~numpy.isnan(back[:, 0])]]))
        roff = numpy.concatenate([[0], numpy.cumsum([len(r) for r in rows])]).astype(numpy.int64)
        start = numpy.asarray([cells[int(res['i'][e])][4] for e in edge])
        t3 = time.perf_counter()
        red = reduce_rows_of(roff, numpy.vstack(rows), n_t, tol=tol, start=start)
        t4 = time.perf_counter()
        t_back, t_pairs, t_reduce = t_back + (t1 - t0) + (t3 - t2), t_pairs + t2 - t1, t_reduce + t4 - t3
        cells = [(int(res['j'][e]) - len(cells), red.rows[red.row_off[n]:red.row_off[n + 1]], nxt[int(res['i'][e])][0], nxt[int(res['i'][e])][1],
                  red.point[n]) for n, e in enumerate(edge)]
        per_step.append(len(cells))
    return per_step, t_pairs, t_back, t_reduce


def main():
    from transition_bench import solve
    from ppopt_amd import _lib, invariance, reach
    from ppopt_amd.region_merge import solution_rows
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='c2,c3_l4,c3')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--max-cells', type=int, default=1 << 18)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'forward_bench.json'))
    args = ap.parse_args()
    out = []
    for name in args.cases.split(','):
        sol, plant = solve(name)
        n_t, tol = sol.theta_dim(), 1e-8
        off, ef, void = solution_rows(sol.critical_regions, n_t, 'forward_bench')
        _, _, xlaw = sol._stacked()
        live = [i for i in range(len(sol)) if i not in set(void)]
        coff = numpy.concatenate([[0], numpy.cumsum(numpy.diff(off)[live])]).astype(numpy.int64)
        crow = numpy.vstack([ef[off[i]:off[i + 1]] for i in live])
        xs = _lib.merge_regions(coff, crow)[0]
        xs = numpy.where(numpy.isfinite(xs), xs, 0.0)
        for plant_name, scale in (('own', 1.0), ('mismatched', MISMATCH)):
            A = scale * numpy.asarray(plant['A'], dtype=float)
            B = numpy.asarray(plant['B'], dtype=float).reshape(n_t, -1)
            g = sol.transition_graph(A, B, plant['inputs'])
            Phi, phi = invariance.closed_loop_maps(xlaw, A, B, numpy.asarray(plant['inputs']))
            succ = [g.successors(i) for i in range(len(sol))]
            loop = lambda: reach.forward_cells(off, ef, Phi, phi, n_t, succ, coff, crow, live, cell_point=xs, tol=tol, max_steps=args.steps,
                                               max_cells=args.max_cells)
            comp = lambda: composition(off, ef, Phi, phi, n_t, succ, live, xs, tol, args.steps)
            got = loop()                       # the warm-up calls
            rec = {'case': name, 'plant': plant_name, 'A_scale': scale, 'n_theta': n_t, 'regions': len(sol), 'edges': int(len(g.indices)),
                   'steps': got.steps, 'status': got.status}
            if got.status not in ('DONE', 'EMPTY'):      # a refusal: the composition has no cap to stop at; the figures of the completed steps only
                rec['note'] = 'refused: only the device-resident loop was timed'
                parts = None
            else:
                parts = comp()
            walls, comp_walls = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                got = loop()
                walls.append((time.perf_counter() - t0) * 1e3)
                if parts is not None:
                    t0 = time.perf_counter()
                    parts = comp()
                    comp_walls.append((time.perf_counter() - t0) * 1e3)
            st = got.stats
            step_ms = sum(st['step_ms'])
            rec.update({'cells': len(got), 'cells_per_step': st['cells_per_step'], 'items': st['items'], 'lps': st['lps'],
                        'pivots_per_lp': st['pivots'] / max(1, st['lps']), 'wide_runs': st['wide'], 'wide_cells': int(got.wide.sum()),
                        'device_ms_per_step': st['step_ms'], 'device_ms_steps': step_ms, 'device_ns_per_lp': 1e6 * step_ms / max(1, st['lps']),
                        'call_ms': st.get('call_ms', 0.0), 'wall_ms': float(numpy.median(walls)), 'wall_ms_all': walls, 'repeats': args.repeats})
            if parts is not None:
                rec.update({'composition_wall_ms': float(numpy.median(comp_walls)), 'composition_wall_ms_all': comp_walls,
                            'composition_cells_per_step': parts[0], 'composition_pairs_ms': parts[1] * 1e3, 'composition_host_ms': parts[2] * 1e3,
                            'composition_reduce_ms': parts[3] * 1e3})
            print(json.dumps(rec), flush=True)
            out.append(rec)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as fh:
                json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
