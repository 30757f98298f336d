"""Removing redundant rows (geometry.reduce) on pieces the drivers produce: rows before and after, LPs and pivots per LP,
device time in sum and per LP, wall time, and how many pieces the volume pass cannot answer before and after the reduction.

    python tools/reduce_bench.py [--out profiles/reduce_bench.json] [--cases c3_l4,c3,mplp]

Cases: the pieces of exit_sets on the four-level config 3 and on the complete config 3 (each under its own plant), reduced in one call
(ExitSets.reduced) and round by round (reduce_rows=True); the pieces of remove_overlaps on the degenerate mpLP of
tests/test_gpu_overlap.py (DESIGN §3.19 has no measured mpLP of its own; this is the solved mpLP its tests use), reduced as a finished
solution (Solution.reduce_rows) and round by round.  No speed threshold is set; the yardstick printed beside each result is the
25.8 to 79 ns per LP of k_exit_split, the same engine on the same rows.
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

YARDSTICK = 'k_exit_split: 25.8 to 79 ns per LP (DESIGN §3.21)'


def unanswered(volumes) -> int:
    return int(numpy.isnan(volumes.piece).sum())


def record(case, how, rows_before, rows_after, pieces, lps, pivots, device_ms, wall_ms, no_volume_before, no_volume_after, **more):
    rec = {'case': case, 'how': how, 'pieces': pieces, 'rows_before': rows_before, 'rows_after': rows_after, 'lps': lps,
           'pivots_per_lp': pivots / max(1, lps) if pivots is not None else None, 'device_ms': device_ms,
           'device_ns_per_lp': 1e6 * device_ms / max(1, lps), 'wall_ms': wall_ms, 'pieces_without_volume_before': no_volume_before,
           'pieces_without_volume_after': no_volume_after, 'yardstick': YARDSTICK}
    rec.update(more)
    print(json.dumps(rec), flush=True)
    return rec


def exit_case(name):
    from transition_bench import solve
    sol, plant = solve(name)
    g = sol.transition_graph(plant['A'], plant['B'], plant['inputs'])
    plain = sol.exit_sets(plant['A'], plant['B'], plant['inputs'], graph=g)
    before = unanswered(plain.volumes())
    plain.reduced()                                                            # warm pools
    t0 = time.perf_counter()
    after = plain.reduced()
    wall = (time.perf_counter() - t0) * 1e3
    from ppopt_amd.geometry.reduce import reduce_rows_of
    r = reduce_rows_of(plain.piece_off, plain.piece_rows, sol.theta_dim(), tol=plain.tol)
    out = [record(name, 'ExitSets.reduced()', int(plain.piece_off[-1]), int(after.piece_off[-1]), len(after), r.stats['lps'], r.stats['pivots'],
                  after.stats['reduce_ms'], wall, before, unanswered(after.volumes()), thin=int(r.stats['thin']), wide=int(r.stats['wide']),
                  max_rows_before=int(numpy.diff(plain.piece_off).max()) if len(plain) else 0,
                  max_rows_after=int(numpy.diff(after.piece_off).max()) if len(after) else 0)]
    t0 = time.perf_counter()
    during = sol.exit_sets(plant['A'], plant['B'], plant['inputs'], graph=g, reduce_rows=True)
    wall = (time.perf_counter() - t0) * 1e3
    st = during.stats
    out.append(record(name, 'exit_sets(reduce_rows=True)', int(plain.piece_off[-1]), int(during.piece_off[-1]), len(during), st['reduce_lps'], None,
                      st['reduce_ms'], wall, before, unanswered(during.volumes()), rows_removed=st['rows_removed'], split_lps=st['lps'],
                      split_lps_plain=plain.stats['lps'], split_device_ms=sum(st['round_ms']), split_device_ms_plain=sum(plain.stats['round_ms']),
                      wall_ms_plain=plain.stats['wall_ms'], max_item_rows=st['max_item_rows'], max_item_rows_plain=plain.stats['max_item_rows']))
    return out


def overlap_case(name):
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if name != 'mplp':
            raise KeyError(name)
        from test_gpu_overlap import degenerate_mplp
        prog = degenerate_mplp()
        sol = solve_mpqp(prog, mpqp_algorithm.combinatorial)
    plain = sol.remove_overlaps()
    rows = lambda s: sum(len(r.E) for r in s.critical_regions)
    plain.reduce_rows()                                                        # warm pools
    t0 = time.perf_counter()
    late = plain.reduce_rows()
    wall = (time.perf_counter() - t0) * 1e3
    s = late.reduce_info['stats']
    out = [record(name, 'Solution.reduce_rows()', rows(plain), rows(late), len(late), s['lps'], s['pivots'], s['device_ms'], wall, None, None,
                  regions=len(sol), thin=s['thin'], wide=s['wide'])]
    t0 = time.perf_counter()
    red = sol.remove_overlaps(reduce_rows=True)
    wall = (time.perf_counter() - t0) * 1e3
    st = red.overlap_info['stats']
    out.append(record(name, 'remove_overlaps(reduce_rows=True)', rows(plain), rows(red), len(red), st['reduce_lps'], None, st['reduce_ms'], wall, None, None,
                      regions=len(sol), rows_removed=st['rows_removed'], wall_ms_plain=plain.overlap_info['stats']['wall_ms']))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='c3_l4,c3,mplp')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reduce_bench.json'))
    args = ap.parse_args()
    out = []
    for name in args.cases.split(','):
        out.extend(exit_case(name) if name.startswith('c') else overlap_case(name))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
