"""The backward exit cells (Solution.invariant_set) on solved workloads, against the host-driven composition of the calls the
package had before: per step transition_pairs on regions + cells for the item statuses, exit_sets.pulled_back_rows on the host, and
reduce_rows_of for the kept rows.  Both start from the same transition graph and exit sets, run in the same process after one warm-up
call each, alternating, and the medians of the wall times are recorded with steps, items, LPs, pivots per LP, cells, device ns per LP and
device ms per step.

    python tools/invariant_bench.py [--out profiles/invariant_bench.json] [--cases c2,c3_l4,c3] [--repeats 5] [--max-steps 64]
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


def composition(off, ef, Phi, phi, n_t, pred, es, tol, max_steps):
    """the iteration driven from the host: (cells per step, seconds in transition_pairs, in the host's pull-back, in reduce_rows_of)"""
    from ppopt_amd import exit_sets as ex, transition as tr
    from ppopt_amd.geometry.reduce import reduce_rows_of
    polys = numpy.split(ef, off[1:-1])
    R = len(polys)
    cells = [(int(s), es.rows_of(k)) for k, s in enumerate(es.source)]
    per_step, t_pairs, t_back, t_reduce = [len(cells)], 0.0, 0.0, 0.0
    for _ in range(max_steps):
        pa = [int(i) for s, _ in cells for i in pred[s]]
        pb = [R + n for n, (s, _) in enumerate(cells) for _ in pred[s]]
        if not pa:
            break
        t0 = time.perf_counter()
        aoff = numpy.concatenate([off, off[-1] + numpy.cumsum([len(r) for _, r in cells])]).astype(numpy.int64)
        aef = numpy.vstack([ef] + [r for _, r in cells])
        P = numpy.concatenate([Phi, numpy.tile(numpy.eye(n_t), (len(cells), 1, 1))])
        p = numpy.concatenate([phi, numpy.zeros((len(cells), n_t))])
        res = tr.transition_pairs(aoff, aef, P, p, n_t, tol=tol, pairs=(pa, pb))
        t1 = time.perf_counter()
        # transition_pairs answers sorted by (i, j); the items go by parent cell, then by region
        edge = numpy.flatnonzero(res['status'] != tr.NO_EDGE)
        edge = edge[numpy.lexsort((res['i'][edge], res['j'][edge]))]
        if not len(edge):
            t_pairs += t1 - t0
            break
        rows = []
        for e in edge:
            i, q = int(res['i'][e]), int(res['j'][e]) - R
            back = ex.pulled_back_rows(cells[q][1], Phi[i], phi[i])
            rows.append(numpy.vstack([polys[i], back[~numpy.isnan(back[:, 0])]]))
        t2 = time.perf_counter()
        roff = numpy.concatenate([[0], numpy.cumsum([len(r) for r in rows])]).astype(numpy.int64)
        red = reduce_rows_of(roff, numpy.vstack(rows), n_t, tol=tol, start=res['witness'][edge])
        t3 = time.perf_counter()
        t_pairs, t_back, t_reduce = t_pairs + t1 - t0, t_back + t2 - t1, t_reduce + t3 - t2
        cells = [(int(res['i'][e]), red.rows[red.row_off[n]:red.row_off[n + 1]]) for n, e in enumerate(edge)]
        per_step.append(len(cells))
    return per_step, t_pairs, t_back, t_reduce


def main():
    from transition_bench import solve
    from ppopt_amd import invariance, invariant_set as inv
    from ppopt_amd.region_merge import solution_rows
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='c2,c3_l4,c3')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--max-steps', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'invariant_bench.json'))
    args = ap.parse_args()
    out = []
    for name in args.cases.split(','):
        sol, plant = solve(name)
        n_t, tol = sol.theta_dim(), 1e-8
        g = sol.transition_graph(plant['A'], plant['B'], plant['inputs'])
        try:
            es = sol.exit_sets(plant['A'], plant['B'], plant['inputs'], graph=g, reduce_rows=True)
        except ValueError as e:              # the exit pieces do not allow it (the 256-row limit of a piece)
            print(json.dumps({'case': name, 'skipped': str(e)}), flush=True)
            out.append({'case': name, 'skipped': str(e)})
            continue
        off, ef, void = solution_rows(sol.critical_regions, n_t, 'invariant_bench')
        _, _, xlaw = sol._stacked()
        Phi, phi = invariance.closed_loop_maps(xlaw, numpy.asarray(plant['A'], dtype=float), numpy.asarray(plant['B'], dtype=float).reshape(n_t, -1),
                                               numpy.asarray(plant['inputs']))
        pred = [g.predecessors(j) for j in range(len(sol))]
        loop = lambda: inv.backward_exit_cells(off, ef, Phi, phi, n_t, pred, es.piece_off, es.piece_rows, es.source, tol=tol, max_steps=args.max_steps,
                                               void=void)
        comp = lambda: composition(off, ef, Phi, phi, n_t, pred, es, tol, args.max_steps)
        got, parts = loop(), comp()            # the warm-up calls
        walls, comp_walls = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            got = loop()
            walls.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            parts = comp()
            comp_walls.append((time.perf_counter() - t0) * 1e3)
        st = got.stats
        step_ms = sum(st['step_ms'])
        rec = {'case': name, 'n_theta': n_t, 'regions': len(sol), 'edges': int(len(g.indices)), 'exit_pieces': len(es), 'steps': got.steps,
               'status': got.status, 'converged': got.converged, 'cells': len(got), 'cells_per_step': st['cells_per_step'], 'items': st['items'],
               'lps': st['lps'], 'pivots_per_lp': st['pivots'] / max(1, st['lps']), 'wide_runs': st['wide'], 'wide_cells': int(got.wide.sum()),
               'device_ms_per_step': st['step_ms'], 'device_ms_steps': step_ms, 'device_ns_per_lp': 1e6 * step_ms / max(1, st['lps']),
               'call_ms': st.get('call_ms', 0.0), 'wall_ms': float(numpy.median(walls)), 'wall_ms_all': walls, 'composition_wall_ms': float(numpy.median(comp_walls)),
               'composition_wall_ms_all': comp_walls, 'composition_cells_per_step': parts[0], 'composition_pairs_ms': parts[1] * 1e3,
               'composition_pull_back_ms': parts[2] * 1e3, 'composition_reduce_ms': parts[3] * 1e3, 'repeats': args.repeats}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
