"""Merged regions against the union of their members, exactly: Solution.merge_regions on the cases of
tests/merge_cases.py (several law groups, holes, thin cells, overlapping sources, n_theta up to 16, regions of more than 128 rows) under
the difference recursion of tests/merge_exact_reference.py, against the CPU reference merger with no case exempt, and the two library
calls on their own (feasible points and boxes; row masks, verdict and t_max of every pair the reference tests) against HiGHS.  Then
Solution.compare(merged, source) pair by pair against HiGHS's radii, on the cases and on 14 regions of the complete c3
(tests/golden/merge_c3_groups.npz), where a wrong radius once read as a union that is none."""
import os

import numpy
import pytest

import merge_cases
import merge_exact_reference as exact
import region_merge_reference as ref
from conftest import GOLDEN
from ppopt_amd import _lib
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.region_merge import mask_rows
from ppopt_amd.solution import Solution
from test_region_merge_cpu import _canonical

pytestmark = pytest.mark.gpu

TOL = 1e-8
NAMES = sorted(merge_cases.CASES)
_DEVICE = {}


def _device(name):
    if name not in _DEVICE:
        _DEVICE[name] = merge_cases.build(name).merge_regions()
    return _DEVICE[name]


def _assert_exact_unions(src, merged, label):
    worst = (0.0, 0.0)
    for r in merged.critical_regions:
        if len(r.members) > 1:
            out, miss = exact.union_defect(merge_cases.rows_of(r), [merge_cases.rows_of(src.critical_regions[i]) for i in r.members], TOL)
            worst = (max(worst[0], out), max(worst[1], miss))
            assert out <= 10 * TOL and miss <= 10 * TOL, (label, r.members, out, miss)
    print(label, 'largest outside, missing:', worst)


def _assert_equals_reference(dev, want):
    assert [r.members for r in dev.critical_regions] == [r.members for r in want.critical_regions]
    for a, b in zip(dev.critical_regions, want.critical_regions):
        assert a.E.shape == b.E.shape, a.members
        numpy.testing.assert_allclose(_canonical(a.E, a.f), _canonical(b.E, b.f), rtol=0, atol=1e-12)
        numpy.testing.assert_array_equal(a.A, b.A)
        numpy.testing.assert_array_equal(a.b, b.b)


@pytest.mark.parametrize('name', NAMES)
def test_merged_regions_are_the_unions_of_their_members(name):
    """No piece of a merged region fatter than 10 tol = 1e-7 lies outside its members, and no such piece of a member outside the region.
    The rule itself allows tol max(1, |o|) per envelope row (|o| <= 1.3 here) plus t* <= tol per merge.  The CPU reference's largest
    value on these cases is 0: no piece fatter than tol = 1e-8 anywhere (pieces up to tol are not measured, the recursion stops there),
    a factor 10 under the bound."""
    _assert_exact_unions(merge_cases.build(name), _device(name), name)


@pytest.mark.parametrize('name', NAMES)
def test_device_equals_the_reference(name):
    want, info = merge_cases.reference(name)
    assert info['knife'] == 0        # test_merge_exact_cpu.py holds the cases to that: nothing is exempt here
    dev = _device(name)
    _assert_equals_reference(dev, want)
    assert len(dev) < len(merge_cases.build(name))


def _stage_regions(name):
    """unit rows of every region the reference handles: the source's regions, then every union it tested as a side of a pair; and the
    tested pairs as indices into that list"""
    src = merge_cases.build(name)
    n_t = numpy.asarray(src.critical_regions[0].E).shape[1]
    regions = [ref._unit(r.E, r.f, n_t)[0] for r in src.critical_regions]
    index = {}
    pairs = []
    for rp, rq, va, vb, ok in merge_cases.reference(name)[1]['tested']:
        for rows in (rp, rq):
            if id(rows) not in index:
                hit = next((k for k, u in enumerate(regions) if u.shape == rows.shape and numpy.array_equal(u, rows)), None)
                if hit is None:
                    hit = len(regions)
                    regions.append(rows)
                index[id(rows)] = hit
        pairs.append((index[id(rp)], index[id(rq)], va, vb, ok))
    return regions, pairs, n_t


def _offsets(regions):
    return numpy.concatenate([[0], numpy.cumsum([len(u) for u in regions])]).astype(numpy.int64)


@pytest.mark.parametrize('name', NAMES)
def test_region_stage_against_highs(name):
    """_lib.merge_regions alone: every region is found non-empty, its point satisfies every row within tol, and its box is HiGHS's
    within 1e-9 (1 + |bound|), thin and grown regions and the unions of later rounds included"""
    regions, _, n_t = _stage_regions(name)
    xs, box, status, stats = _lib.merge_regions(_offsets(regions), numpy.vstack(regions))
    assert stats['capped'] == 0
    for k, u in enumerate(regions):
        assert status[k] == 0, k
        assert numpy.max(u[:, 1:] @ xs[k] - u[:, 0]) <= TOL, k
        lo, hi = ref._box(u, n_t)
        for got, want in ((box[k, 0], lo), (box[k, 1], hi)):
            fin = numpy.isfinite(want)
            assert numpy.array_equal(got[~fin], want[~fin]), k
            assert numpy.all(numpy.abs(got[fin] - want[fin]) <= 1e-9 * (1.0 + numpy.abs(want[fin]))), (k, got, want)


def _bits(words, m):
    out = numpy.zeros(m, dtype=bool)
    out[mask_rows(words, m)] = True
    return out


@pytest.mark.parametrize('name', NAMES)
def test_pair_stage_against_highs(name):
    """_lib.merge_pairs alone on every candidate pair the reference forms: both row masks equal the reference's valid rows, the verdict
    its pair test, t_max <= tol exactly when the pair is convex; the same from HiGHS's boxes and Chebyshev centres as from the device's
    points and boxes, and the same bits per pair from a permuted pair list"""
    regions, pairs, n_t = _stage_regions(name)
    assert pairs
    off, rows = _offsets(regions), numpy.vstack(regions)
    xs, box, status, _ = _lib.merge_regions(off, rows)
    assert not status.any()
    pa, pb = [p for p, _, _, _, _ in pairs], [q for _, q, _, _, _ in pairs]
    env_a, env_b, verdict, t_max, stats = _lib.merge_pairs(off, rows, xs, box, pa, pb, TOL)
    assert stats['capped'] == 0 and stats['pairs'] == len(pairs)
    for k, (p, q, va, vb, ok) in enumerate(pairs):
        assert numpy.array_equal(_bits(env_a[k], len(regions[p])), va), (k, p, q)
        assert numpy.array_equal(_bits(env_b[k], len(regions[q])), vb), (k, p, q)
        assert bool(verdict[k]) == ok, (k, p, q, t_max[k])
        assert (t_max[k] <= TOL) == ok, (k, p, q, t_max[k])
    # no bit beyond a region's rows
    for k, (p, q, _, _, _) in enumerate(pairs):
        for words, m in ((env_a[k], len(regions[p])), (env_b[k], len(regions[q]))):
            bits = numpy.unpackbits(numpy.ascontiguousarray(words, dtype='<u8').view(numpy.uint8), bitorder='little')
            assert not bits[m:].any(), (k, p, q)
    # exact inputs instead of the region stage's: HiGHS's boxes, and the Chebyshev centre as the feasible point
    used = sorted(set(pa) | set(pb))
    xs_h, box_h = xs.copy(), box.copy()
    for i in used:
        u = regions[i]
        lp = ref.linprog(numpy.append(numpy.zeros(n_t), -1.0), A_ub=numpy.column_stack([u[:, 1:], numpy.ones(len(u))]), b_ub=u[:, 0],
                         bounds=[(None, None)] * n_t + [(0, 1.0)], method='highs')
        assert lp.status == 0
        xs_h[i] = lp.x[:n_t]
        box_h[i, 0], box_h[i, 1] = ref._box(u, n_t)
    ea, eb, vd, _, _ = _lib.merge_pairs(off, rows, xs_h, box_h, pa, pb, TOL)
    assert numpy.array_equal(ea, env_a) and numpy.array_equal(eb, env_b) and numpy.array_equal(vd, verdict)
    # a permuted pair list
    perm = numpy.random.default_rng(5).permutation(len(pairs))
    ea, eb, vd, tm, _ = _lib.merge_pairs(off, rows, xs, box, [pa[i] for i in perm], [pb[i] for i in perm], TOL)
    assert numpy.array_equal(ea, env_a[perm]) and numpy.array_equal(eb, env_b[perm]) and numpy.array_equal(vd, verdict[perm])
    assert numpy.array_equal(tm <= TOL, t_max[perm] <= TOL)


# ---- the law groups of the complete c3 whose merged regions were not the unions of their members ---------------------
def _c3_groups():
    g = numpy.load(os.path.join(GOLDEN, 'merge_c3_groups.npz'))
    off, rows, laws = g['row_off'], g['rows'], g['laws']
    n_t = rows.shape[1] - 1
    regs = []
    for k in range(len(off) - 1):
        u = rows[off[k]:off[k + 1]]
        regs.append(CriticalRegion(laws[k][:, :n_t].copy(), laws[k][:, n_t:].copy(), numpy.zeros((0, n_t)), numpy.zeros((0, 1)),
                                   u[:, 1:].copy(), u[:, :1].copy(), []))
    return Solution(merge_cases._Prog(n_t), regs, point_location_tolerance=1e-5)


def _assert_compare_matches_highs(src, merged, label, own_gap=0.0):
    """Solution.compare(merged, source), pair by pair: the radius of every candidate is the Chebyshev radius of the stacked rows within
    1e-9 (1 + |r|) (the tolerance of the boxes above: both are optima of LPs over the same rows), so a pair meets exactly when HiGHS
    says so; every member meets its own region, with a gap of at most ``own_gap`` (0: a member's law is its region's law to the bit
    in the generated sources)"""
    g = merged.compare(src)
    assert g.wide == 0
    owner = {i: k for k, r in enumerate(merged.critical_regions) for i in r.members}
    met = set()
    for k in range(len(g.i)):
        i, j = int(g.i[k]), int(g.j[k])
        (Ei, fi), (Ej, fj) = merge_cases.rows_of(merged.critical_regions[i]), merge_cases.rows_of(src.critical_regions[j])
        want = exact.chebyshev_radius(numpy.vstack([Ei, Ej]), numpy.concatenate([fi, fj]))
        assert abs(g.radius[k] - want) <= 1e-9 * (1.0 + abs(want)), (label, i, j, g.radius[k], want)
        if abs(want - TOL) > 1e-9:
            assert bool(g.meets[k]) == (want > TOL), (label, i, j, g.radius[k], want)
        if owner[j] == i and g.meets[k]:
            met.add(j)
            assert g.gap[k] <= own_gap, (label, i, j, g.gap[k])
    fat = {j for j, r in enumerate(src.critical_regions) if exact.chebyshev_radius(*merge_cases.rows_of(r)) > 2 * TOL}
    assert fat <= met, (label, sorted(fat - met))
    assert not set(g.unmatched_b.tolist()) & fat


@pytest.mark.parametrize('name', NAMES)
def test_compare_of_merged_and_source_against_highs(name):
    """The rows of a merged region stacked on the rows of a member hold exact copies and nearly parallel rows: the radius LPs of
    Solution.compare on them, which is how DESIGN §3.26 came to report unions that were none"""
    _assert_compare_matches_highs(merge_cases.build(name), _device(name), name)


def test_regions_of_the_complete_c3():
    """Regions of the complete c3 (geometric driver, outputs 0 and 1): members 1108 and 1639 and 1119 and 1652 of two merged regions, the
    same-law regions that touch 1639, and region 5794 of another law.  Solution.compare reported the first union as only touching its
    member 1639 (radius -1.7e-12 for 0.034) and the second as overlapping 5794 (radius 0.045 for -0.37): the merged regions are exact
    unions, the radius LPs were wrong (csrc/simplex.hpp, the ratio test)."""
    g = numpy.load(os.path.join(GOLDEN, 'merge_c3_groups.npz'))
    index = g['source_index'].tolist()
    src = _c3_groups()
    merged = src.merge_regions()
    groups = [[index[i] for i in r.members] for r in merged.critical_regions if len(r.members) > 1]
    assert [1108, 1639] in groups and [1119, 1652] in groups
    _assert_exact_unions(src, merged, 'c3 regions')
    want, info = ref.merge_reference(src)
    assert info['knife'] == 0
    _assert_equals_reference(merged, want)
    # laws of one group agree with the group's first within law_tol (1 + max |law|) per entry, two members within twice that, so
    # |dA theta + db| <= 2 law_tol (1 + max |law|) (1 + sum |theta_i|), and |theta_i| <= 5 on c3
    laws, n_t = g['laws'], g['rows'].shape[1] - 1
    assert numpy.max(numpy.abs(g['rows'][:, 0])) <= 5.0 * numpy.sqrt(n_t)
    own_gap = 2 * TOL * (1.0 + numpy.max(numpy.abs(laws))) * (1.0 + 5.0 * n_t)
    _assert_compare_matches_highs(src, merged, 'c3 regions', own_gap)
    cmp = merged.compare(src)
    pair = {(index[merged.critical_regions[int(i)].members[0]], index[int(j)]): k for k, (i, j) in enumerate(zip(cmp.i, cmp.j))}
    assert abs(cmp.radius[pair[(1108, 1639)]] - 0.03410417091367) <= 1e-12 and cmp.meets[pair[(1108, 1639)]]
    assert (1119, 5794) not in pair or not cmp.meets[pair[(1119, 5794)]]
    assert cmp.max_gap <= own_gap        # nothing of the other law meets a merged region of this one
