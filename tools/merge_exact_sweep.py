"""Every merged region of a solved workload against the union of its members, exactly, in two sweeps (HiGHS):

  union    the difference recursion of tests/merge_exact_reference.py on each result region of Solution.merge_regions that has more
           than one member: a defect is a piece fatter than 10 tol outside the members, or such a piece of a member outside the region;
  compare  Solution.compare(merged, source), the call that reported DESIGN §3.26: the radius of every pair it says meets, and of every
           merged region with each of its own members, against the Chebyshev radius of the stacked rows; a wrong pair differs by more
           than 1e-9 (1 + |radius|).

    python tools/merge_exact_sweep.py [--case c3_graph | c3_geometric | c3_l4] [--out profiles/merge_exact_sweep.json]
                                      [--save state.npz | --load state.npz]
                                      [--fixture tests/golden/merge_c3_groups.npz [--fixture-sources 1639,5794]]

The solve, the merge and the comparison need the device; the sweeps do not: --save writes the source's unit rows and laws, the merged
regions and the comparison's pairs, --load runs the sweeps on such a file.  --fixture writes the regions behind the findings as unit
rows and laws on the merged outputs: of a defective union its members; of a wrong pair the merged region's members and the source
region, and where that one is a member, the regions of its law group that touch it (--fixture-sources keeps the wrong pairs of these
source regions only; the committed fixture is that of 1639 and 5794 on c3_geometric): the input of
tests/test_gpu_merge_exact.py::test_regions_of_the_complete_c3.
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

TOL = 1e-8


def solve_and_merge(case):
    """the state of a sweep: the source's unit rows and laws on the merged outputs, and the merged regions with several members"""
    from ppopt_amd.region_merge import law_groups, law_of, unit_rows
    if case == 'c3_geometric':      # the source of DESIGN §3.26 (tools/compare_bench.py, case c3): 26 pairs of its regions overlap
        import warnings
        import bench
        from ppopt_amd.mp_solvers import mpqp_hip_geometric
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            src = mpqp_hip_geometric.solve(bench.build_program('c3'))
        outputs = [0, 1]
    else:
        from merge_bench import OUTPUTS, solve
        src = solve(case)
        outputs = OUTPUTS[case]
    merged = src.merge_regions(outputs=outputs)
    n_t = src.theta_dim()
    rows = [unit_rows(r.E, r.f, n_t)[0] for r in src.critical_regions]
    laws = numpy.asarray([law_of(r, outputs, n_t) for r in src.critical_regions])
    multi = [r for r in merged.critical_regions if len(r.members) > 1]
    g = merged.compare(src, outputs=outputs)
    owner = numpy.empty(len(src), dtype=numpy.int64)
    for k, r in enumerate(merged.critical_regions):
        owner[r.members] = k
    take = g.meets | (owner[g.j] == g.i)
    m_rows = [unit_rows(r.E, r.f, n_t)[0] for r in multi]
    cum = lambda parts: numpy.concatenate([[0], numpy.cumsum([len(p) for p in parts])]).astype(numpy.int64)
    return {'case': numpy.asarray(case), 'outputs': numpy.asarray(outputs), 'row_off': cum(rows), 'rows': numpy.vstack(rows), 'laws': laws,
            'groups': law_groups(laws, TOL), 'regions_after': numpy.asarray(len(merged)),
            'member_off': cum([r.members for r in multi]), 'members': numpy.concatenate([r.members for r in multi]).astype(numpy.int64),
            'merged_row_off': cum(m_rows), 'merged_rows': numpy.vstack(m_rows),
            'stats': numpy.asarray(json.dumps(merged.merge_info['stats'])),
            'multi_index': numpy.asarray([k for k, r in enumerate(merged.critical_regions) if len(r.members) > 1], dtype=numpy.int64),
            'owner': owner, 'cmp_i': g.i[take], 'cmp_j': g.j[take], 'cmp_radius': g.radius[take], 'cmp_gap': g.gap[take],
            'cmp_flag': g.flag[take], 'cmp_unmatched_b': g.unmatched_b, 'cmp_max_gap': numpy.asarray(g.max_gap),
            'cmp_stats': numpy.asarray(json.dumps(g.stats))}


def _poly(rows, off, k):
    r = rows[off[k]:off[k + 1]]
    return r[:, 1:], r[:, 0]


def sweep(state, tol=TOL):
    """(record, defects): a defect is a merged region with a piece outside its members or a piece of a member missing above 10 tol"""
    import merge_exact_reference as exact
    t0 = time.perf_counter()
    n_multi = len(state['member_off']) - 1
    defects, worst_out, worst_miss = [], 0.0, 0.0
    for k in range(n_multi):
        mem = state['members'][state['member_off'][k]:state['member_off'][k + 1]]
        out, miss = exact.union_defect(_poly(state['merged_rows'], state['merged_row_off'], k),
                                       [_poly(state['rows'], state['row_off'], i) for i in mem], tol)
        worst_out, worst_miss = max(worst_out, out), max(worst_miss, miss)
        if out > 10 * tol or miss > 10 * tol:
            defects.append({'merged_multi': k, 'members': [int(i) for i in mem], 'outside': float(out), 'missing': float(miss),
                            'rows': int(state['merged_row_off'][k + 1] - state['merged_row_off'][k])})
    rec = {'case': str(state['case']), 'outputs': [int(o) for o in state['outputs']], 'tol': tol, 'bound': 10 * tol,
           'regions_before': int(len(state['row_off']) - 1), 'regions_after': int(state['regions_after']), 'multi_member_regions': n_multi,
           'largest_outside': float(worst_out), 'largest_missing': float(worst_miss), 'defective': len(defects), 'defects': defects,
           'sweep_wall_s': time.perf_counter() - t0, 'merge_stats': json.loads(str(state['stats']))}
    return rec, defects


def _merged_poly(state, i):
    """rows of result region i: a union's own rows, or its single member's"""
    k = numpy.flatnonzero(state['multi_index'] == i)
    if len(k):
        return _poly(state['merged_rows'], state['merged_row_off'], int(k[0]))
    return _poly(state['rows'], state['row_off'], int(numpy.flatnonzero(state['owner'] == i)[0]))


def sweep_compare(state):
    """(record, wrong pairs) of the comparison's radii against HiGHS"""
    import merge_exact_reference as exact
    t0 = time.perf_counter()
    wrong, own_gap = [], 0.0
    for k in range(len(state['cmp_i'])):
        i, j, r = int(state['cmp_i'][k]), int(state['cmp_j'][k]), float(state['cmp_radius'][k])
        (Ei, fi), (Ej, fj) = _merged_poly(state, i), _poly(state['rows'], state['row_off'], j)
        want = exact.chebyshev_radius(numpy.vstack([Ei, Ej]), numpy.concatenate([fi, fj]))
        own = int(state['owner'][j]) == i
        if own and numpy.isfinite(state['cmp_gap'][k]):
            own_gap = max(own_gap, float(state['cmp_gap'][k]))
        if not abs(r - want) <= 1e-9 * (1.0 + abs(want)):
            wrong.append({'merged': i, 'source': j, 'own_member': own, 'device_radius': r, 'highs_radius': float(want),
                          'gap': None if numpy.isnan(state['cmp_gap'][k]) else float(state['cmp_gap'][k])})
    rec = {'pairs_checked': int(len(state['cmp_i'])), 'wrong_radius': len(wrong), 'wrong': wrong, 'max_gap': float(state['cmp_max_gap']),
           'largest_gap_to_an_own_member': own_gap, 'unmatched_source_regions': [int(i) for i in state['cmp_unmatched_b']],
           'sweep_wall_s': time.perf_counter() - t0, 'compare_stats': json.loads(str(state['cmp_stats']))}
    return rec, wrong


def touching_in_group(state, j, tol=1e-9):
    """regions of j's law group whose intersection with region j is not emptier than -tol (facet neighbours and overlaps)"""
    import merge_exact_reference as exact
    Ej, fj = _poly(state['rows'], state['row_off'], j)
    hits = []
    for i in numpy.flatnonzero(state['groups'] == state['groups'][j]):
        Ei, fi = _poly(state['rows'], state['row_off'], i)
        if i != j and exact.chebyshev_radius(numpy.vstack([Ej, Ei]), numpy.concatenate([fj, fi])) >= -tol:
            hits.append(int(i))
    return hits


def write_fixture(state, defects, wrong, path):
    keep = [i for d in defects for i in d['members']]
    for w in wrong:
        keep.extend(numpy.flatnonzero(state['owner'] == w['merged']).tolist())
        keep.append(w['source'])
        if w['own_member']:
            keep.extend(touching_in_group(state, w['source']))
    keep = sorted(set(int(i) for i in keep))
    rows = [state['rows'][state['row_off'][i]:state['row_off'][i + 1]] for i in keep]
    numpy.savez_compressed(path, source_index=numpy.asarray(keep, dtype=numpy.int64),
                           row_off=numpy.concatenate([[0], numpy.cumsum([len(r) for r in rows])]).astype(numpy.int64),
                           rows=numpy.vstack(rows), laws=state['laws'][keep])
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='c3_graph')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'merge_exact_sweep.json'))
    ap.add_argument('--save')
    ap.add_argument('--load')
    ap.add_argument('--fixture')
    ap.add_argument('--fixture-sources', default='')
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    if args.load:
        state = dict(numpy.load(args.load))
    else:
        state = solve_and_merge(args.case)
        if args.save:
            os.makedirs(os.path.dirname(os.path.abspath(args.save)), exist_ok=True)
            numpy.savez_compressed(args.save, **state)
    rec, defects = sweep(state)
    rec['compare'], wrong = sweep_compare(state)
    if args.fixture and (defects or wrong):
        only = {int(v) for v in args.fixture_sources.split(',') if v}
        rec['fixture_source_regions'] = write_fixture(state, defects, [w for w in wrong if not only or w['source'] in only], args.fixture)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
