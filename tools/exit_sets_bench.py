"""The exit sets (Solution.exit_sets) on solved workloads: regions, edges, rounds, items, LPs and pivots, pieces, the exit
share of the total volume, device time per round and in sum, wall time, and the CPU reference's time per LP on a sample of regions.

    python tools/exit_sets_bench.py [--out profiles/exit_sets_bench.json] [--cases c2,c3_l4,c3] [--sample 20]
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


def reference_ms_per_lp(sol, plant, graph, es, sample: int):
    """the CPU reference (tests/exit_reference.py, HiGHS) on a seeded sample of regions: (ms per LP, LPs, regions whose pieces differ in
    number from the device's, knife regions among the sample)"""
    import exit_reference as ref
    import transition_reference as tref
    from ppopt_amd import invariance
    from ppopt_amd.region_merge import unit_rows
    n_t = sol.theta_dim()
    polys = [unit_rows(r.E, r.f, n_t)[0] for r in sol.critical_regions]
    _, _, xlaw = sol._stacked()
    Phi, phi = invariance.closed_loop_maps(xlaw, numpy.asarray(plant['A'], dtype=float), numpy.asarray(plant['B'], dtype=float).reshape(n_t, -1),
                                           numpy.asarray(plant['inputs']))
    pick = numpy.random.default_rng(0).choice(len(polys), min(sample, len(polys)), replace=False)
    lps = [0]
    inner = tref.chebyshev

    def counted(rows):
        lps[0] += 1
        return inner(rows)

    tref.chebyshev = counted
    try:
        t0 = time.perf_counter()
        want, knife = ref.exit_reference(polys, Phi, phi, [graph.successors(i) for i in range(len(polys))], 1e-8, regions=pick)
        ms = (time.perf_counter() - t0) * 1e3
    finally:
        tref.chebyshev = inner
    differ = sum(len(es.pieces_of(int(i))) != sum(p[0] == i for p in want) for i in pick if int(i) not in knife)
    return ms / max(1, lps[0]), lps[0], int(differ), len(knife)


def main():
    from transition_bench import solve
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='c2,c3_l4,c3')
    ap.add_argument('--sample', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exit_sets_bench.json'))
    args = ap.parse_args()
    out = []
    for name in args.cases.split(','):
        sol, plant = solve(name)
        g = sol.transition_graph(plant['A'], plant['B'], plant['inputs'])
        sol.exit_sets(plant['A'], plant['B'], plant['inputs'], graph=g)      # warm pools
        t0 = time.perf_counter()
        es = sol.exit_sets(plant['A'], plant['B'], plant['inputs'], graph=g)
        wall = time.perf_counter() - t0
        st = es.stats
        try:
            vol = es.volumes()
            share, undecided = vol.total_share, int(numpy.isnan(vol.piece).sum() + numpy.isnan(vol.region).sum())
        except (ValueError, RuntimeError) as e:      # the limits of the volume pass
            share, undecided = float('nan'), str(e)
        ref_ms, ref_lps, differ, knife = reference_ms_per_lp(sol, plant, g, es, args.sample)
        round_ms = sum(st['round_ms'])
        rec = {'case': name, 'n_theta': sol.theta_dim(), 'regions': len(sol), 'edges': int(len(g.indices)), 'rounds': st['rounds'], 'items': st['items'],
               'lps': st['lps'], 'pivots_per_lp': st['pivots'] / max(1, st['lps']), 'pieces': len(es), 'whole_regions': int(es.whole.sum()),
               'wide': st['wide'], 'max_item_rows': st['max_item_rows'], 'exit_share_of_volume': share, 'volume_undecided': undecided,
               'device_ms_per_round': st['round_ms'], 'device_ms_rounds': round_ms, 'device_ms': st['device_ms'],
               'device_ns_per_lp': 1e6 * round_ms / max(1, st['lps']), 'wall_ms': wall * 1e3, 'host_ms': wall * 1e3 - st['device_ms'],
               'reference_ms_per_lp': ref_ms, 'reference_lps': ref_lps, 'reference_regions_differing': differ, 'reference_knife_regions': knife}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
