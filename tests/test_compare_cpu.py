"""The host side of Solution.compare (ppopt_amd/compare.py) and the CPU reference of its device part; no device."""
import numpy
import pytest

import compare_cases as cases
import compare_reference as ref
from ppopt_amd import Solution, compare as cmp
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.region_merge import MergedRegion

TOL = 1e-8


# ---- the reference on the hand cases ----------------------------------------------------------------------------------------------------
def test_reference_one_d_by_hand():
    """c = 0.5 against c = 0.6, by hand.  Regions of A: [-.75, -.25], [-.25, .25], [.25, .75]; of B: [-.8, -.3], [-.3, .3], [.3, .8].
    right(A) n middle(B) = [.25, .3]: delta = .5 - 2 theta falls from 0 to -0.1, an LP optimum at theta = .3.
    right(A) n right(B) = [.3, .75]: delta = (.5 - 2 theta) - (.6 - 2 theta) = -0.1, a constant row.
    middle n middle: both laws are 0.  right(A) n left(B), and the like: disjoint.  right(B) = [.3, .8] is covered on [.3, .75]: 0.9."""
    pa, la = cases.one_d_by_hand(0.5)
    pb, lb = cases.one_d_by_hand(0.6)
    assert numpy.allclose(pa[2][:, 0] * pa[2][:, 1], [0.75, 0.25]) and numpy.allclose(pb[2][:, 0] * pb[2][:, 1], [0.8, 0.3])
    got = {(i, j): ref.pair_reference(pa[i], pb[j], la[i], lb[j], TOL) for i in range(3) for j in range(3)}
    assert sorted(k for k, v in got.items() if v['meets']) == [(0, 0), (0, 1), (1, 1), (2, 1), (2, 2)]
    assert all(v['knife'] is False for v in got.values())
    lp, const, mid = got[(2, 1)], got[(2, 2)], got[(1, 1)]
    assert abs(lp['radius'] - 0.025) <= 1e-12 and abs(lp['lo'][0] + 0.1) <= 1e-12 and abs(lp['hi'][0]) <= 1e-12 and lp['lps'] == 3
    assert abs(lp['gap'] - 0.1) <= 1e-12 and lp['row'] == 0 and lp['flag'] == 0
    assert abs(const['radius'] - 0.225) <= 1e-12 and const['constant'] == 1 and const['lps'] == 1
    assert abs(const['gap'] - 0.1) <= 1e-15 and const['lo'][0] == const['hi'][0]
    assert mid['gap'] == 0.0 and mid['constant'] == 1
    assert abs(max(v['gap'] for v in got.values() if v['meets']) - 0.1) <= 1e-12
    assert abs((0.75 - 0.3) / (0.8 - 0.3) - 0.9) <= 1e-15


def test_reference_open_cases():
    polys, laws, pairs = cases.open_quadrant()
    got = ref.gap_reference(polys, laws, pairs, TOL)
    q = got[(0, 0)]
    assert q['radius'] == numpy.inf and q['gap'] == numpy.inf and q['row'] == -1 and q['flag'] == 1 and q['lps'] == 1
    c = got[(0, 1)]
    assert abs(c['radius'] - 0.5) <= 1e-12 and abs(c['lo'][0]) <= 1e-12 and abs(c['hi'][0] - 3.0) <= 1e-12 and c['flag'] == 0
    polys, laws, pairs = cases.open_half_strip()
    got = ref.gap_reference(polys, laws, pairs, TOL)
    a, b = got[(0, 1)], got[(2, 1)]
    assert abs(a['radius'] - 0.5) <= 1e-12 and abs(a['lo'][0]) <= 1e-12 and a['hi'][0] == numpy.inf and a['gap'] == numpy.inf and a['flag'] == 1
    assert abs(b['lo'][0]) <= 1e-12 and abs(b['hi'][0] - 1.0) <= 1e-12 and abs(b['gap'] - 1.0) <= 1e-12 and b['flag'] == 0 and b['row'] == 0


def test_reference_ties_go_to_the_lowest_row():
    box = cases.box_rows(2)
    law_i = numpy.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]])       # rows 1 and 2 both reach 1
    got = ref.pair_reference(box, box, law_i, numpy.zeros((3, 3)), TOL)
    assert abs(got['gap'] - 1.0) <= 1e-12 and got['row'] == 1 and got['constant'] == 1 and got['lps'] == 5


# ---- cross_box_pairs ------------------------------------------------------------------------------------------------------------------
def _brute(box_a, usable_a, box_b, usable_b, tol):
    out = []
    for i in numpy.flatnonzero(usable_a):
        for j in numpy.flatnonzero(usable_b):
            if all(min(box_a[i, 1, t], box_b[j, 1, t]) - max(box_a[i, 0, t], box_b[j, 0, t]) > tol for t in range(box_a.shape[2])):
                out.append((int(i), int(j)))
    return out


@pytest.mark.parametrize('n_t', [1, 2, 5])
def test_cross_box_pairs_against_all_pairs(n_t):
    rng = numpy.random.default_rng(7 + n_t)

    def boxes(R):
        lo = rng.uniform(-1.0, 1.0, (R, n_t))
        box = numpy.stack([lo, lo + rng.uniform(0.0, 0.8, (R, n_t))], axis=1)
        open_lo, open_hi = rng.random((R, n_t)) < 0.15, rng.random((R, n_t)) < 0.15
        box[:, 0][open_lo] = -numpy.inf
        box[:, 1][open_hi] = numpy.inf
        return box

    box_a, box_b = boxes(23), boxes(31)
    box_a[6, 0], box_a[6, 1] = -0.25, 0.25
    box_b[3] = box_a[5]                                                   # equal boxes
    box_b[4, 0], box_b[4, 1] = box_a[6, 1], box_a[6, 1] + 0.5             # touching in every coordinate: no overlap above tol
    usable_a, usable_b = rng.random(23) < 0.85, rng.random(31) < 0.85
    usable_a[[5, 6]] = usable_b[[3, 4]] = True
    pa, pb = cmp.cross_box_pairs(box_a, usable_a, box_b, usable_b, TOL)
    want = _brute(box_a, usable_a, box_b, usable_b, TOL)
    assert list(zip(pa.tolist(), pb.tolist())) == want and len(want) > 10
    assert (5, 3) in want and (6, 4) not in want
    assert pa.dtype == pb.dtype == numpy.int64
    none = cmp.cross_box_pairs(box_a, numpy.zeros(23, dtype=bool), box_b, usable_b, TOL)
    assert len(none[0]) == len(none[1]) == 0


def test_cross_box_pairs_whole_space():
    whole = numpy.array([[[-numpy.inf, -numpy.inf], [numpy.inf, numpy.inf]]])
    some = numpy.array([[[0.0, 0.0], [1.0, 1.0]], [[-numpy.inf, 2.0], [0.5, numpy.inf]]])
    pa, pb = cmp.cross_box_pairs(whole, numpy.ones(1, dtype=bool), some, numpy.ones(2, dtype=bool), TOL)
    assert list(zip(pa.tolist(), pb.tolist())) == [(0, 0), (0, 1)]
    pa, pb = cmp.cross_box_pairs(some, numpy.ones(2, dtype=bool), some, numpy.ones(2, dtype=bool), TOL)
    assert list(zip(pa.tolist(), pb.tolist())) == [(0, 0), (1, 1)]


# ---- LawGap aggregation ------------------------------------------------------------------------------------------------------------------
def _law_gap(**kw):
    nan = numpy.nan
    base = dict(n_a=4, n_b=3, tol=TOL, outputs=[0, 1],
                i=numpy.array([0, 0, 1, 1, 2]), j=numpy.array([0, 1, 1, 2, 2]),
                radius=numpy.array([0.5, 0.0, 0.25, 0.125, 1e-9]), gap=numpy.array([0.25, nan, 0.75, 0.75, nan]),
                row=numpy.array([1, -1, 0, 1, -1], dtype=numpy.int32), witness=numpy.zeros((5, 2)), flag=numpy.zeros(5, dtype=numpy.int32),
                usable_a=numpy.array([True, True, True, False]), usable_b=numpy.array([True, True, True]))
    base.update(kw)
    return cmp.LawGap(**base)


def test_law_gap_aggregation():
    g = _law_gap()
    assert g.meets.tolist() == [True, False, True, True, False]
    assert g.max_gap == 0.75 and g.argmax == 2                       # the first of the two pairs that attain it
    assert g.worst(2).tolist() == [2, 3] and g.worst(10).tolist() == [2, 3, 0] and g.worst(0).tolist() == []
    numpy.testing.assert_array_equal(g.gap_of_a, [0.25, 0.75, numpy.nan, numpy.nan])
    numpy.testing.assert_array_equal(g.gap_of_b, [0.25, 0.75, 0.75])
    assert g.unmatched_a.tolist() == [2] and g.unmatched_b.tolist() == []      # region 3 of A is not usable: it is not reported
    assert g.wide == 0 and not g.equal(1.0)                          # region 2 of A has no partner
    full = _law_gap(radius=numpy.array([0.5, 0.0, 0.25, 0.125, 0.5]), gap=numpy.array([0.25, numpy.nan, 0.75, 0.75, 0.0]),
                    row=numpy.array([1, -1, 0, 1, 0], dtype=numpy.int32))
    assert len(full.unmatched_a) == 0 and full.equal(0.75) and not full.equal(0.7499)
    wide = _law_gap(radius=numpy.array([0.5, 0.0, 0.25, 0.125, numpy.inf]), gap=numpy.array([0.25, numpy.nan, 0.75, 0.75, numpy.inf]),
                    flag=numpy.array([0, 0, 0, 0, 1], dtype=numpy.int32))
    assert wide.wide == 1 and wide.max_gap == numpy.inf and wide.argmax == 4 and not wide.equal(numpy.inf)
    assert wide.gap_of_a[2] == numpy.inf and len(wide.unmatched_a) == 0


def test_law_gap_nothing_meets():
    g = _law_gap(gap=numpy.full(5, numpy.nan), row=numpy.full(5, -1, dtype=numpy.int32))
    assert g.max_gap == 0.0 and g.argmax == -1 and g.worst(3).tolist() == []
    assert numpy.all(numpy.isnan(g.gap_of_a)) and g.unmatched_a.tolist() == [0, 1, 2] and g.unmatched_b.tolist() == [0, 1, 2]
    assert not g.equal(1.0)
    empty = _law_gap(i=numpy.zeros(0, dtype=numpy.int64), j=numpy.zeros(0, dtype=numpy.int64), radius=numpy.zeros(0), gap=numpy.zeros(0),
                     row=numpy.zeros(0, dtype=numpy.int32), witness=numpy.zeros((0, 2)), flag=numpy.zeros(0, dtype=numpy.int32))
    assert empty.max_gap == 0.0 and empty.argmax == -1 and empty.wide == 0


# ---- solutions: the output mapping and the refusals -------------------------------------------------------------------------------------
def _region(n_t, n_x, rows=None, merged=False):
    E = numpy.vstack([numpy.eye(n_t), -numpy.eye(n_t)]) if rows is None else numpy.tile(numpy.eye(n_t)[:1], (rows, 1))
    f = numpy.ones((len(E), 1))
    A, b = numpy.arange(n_x * n_t, dtype=float).reshape(n_x, n_t), numpy.arange(n_x, dtype=float).reshape(n_x, 1)
    if merged:
        return MergedRegion(A, b, numpy.zeros((0, n_t)), numpy.zeros((0, 1)), E, f, [], members=[0])
    return CriticalRegion(A, b, numpy.zeros((0, n_t)), numpy.zeros((0, 1)), E, f, [])


def _solution(n_t=2, n_x=4, n=2, kept=None, **kw):
    sol = Solution(None, [_region(n_t, n_x if kept is None else len(kept), merged=kept is not None, **kw) for _ in range(n)])
    if kept is not None:
        sol.merge_info = {'source': None, 'outputs': list(kept), 'members': [[0]] * n, 'stats': {}}
    return sol


def test_output_rows_of_plain_and_merged_solutions():
    plain, merged = _solution(n_x=4), _solution(kept=[3, 1])
    assert cmp.output_rows(plain, None) == [0, 1, 2, 3] and cmp.output_rows(plain, [2, 0]) == [2, 0]
    assert cmp.output_rows(merged, None) == [0, 1]
    assert cmp.output_rows(merged, [1]) == [1] and cmp.output_rows(merged, [3]) == [0] and cmp.output_rows(merged, [1, 3]) == [1, 0]
    n_t, rows_a, rows_b = cmp.check_sources(merged, plain, [1, 3], TOL)
    assert (n_t, rows_a, rows_b) == (2, [1, 0], [1, 3])
    # the laws that reach the device are the requested rows of x on both sides
    la, lb = cmp._laws(merged, rows_a, n_t), cmp._laws(plain, rows_b, n_t)
    assert la.shape == lb.shape == (2, 2, 3)
    numpy.testing.assert_array_equal(la[0], numpy.hstack([merged.critical_regions[0].b, merged.critical_regions[0].A])[[1, 0]])
    numpy.testing.assert_array_equal(lb[0], numpy.hstack([plain.critical_regions[0].b, plain.critical_regions[0].A])[[1, 3]])


@pytest.fixture
def no_device(monkeypatch):
    from ppopt_amd import _lib

    def refuse(*a, **k):
        raise AssertionError('the device was reached')
    for name in ('load', 'merge_regions', 'law_gap_pairs', 'reduce_rows'):
        monkeypatch.setattr(_lib, name, refuse)


def test_compare_refuses_before_any_launch(no_device):
    plain = _solution()
    with pytest.raises(ValueError, match='kept the rows'):
        _solution(kept=[3, 1]).compare(plain, outputs=[0])
    with pytest.raises(ValueError, match='no regions'):
        Solution(None, []).compare(plain)
    with pytest.raises(ValueError, match='no regions'):
        plain.compare(Solution(None, []))
    with pytest.raises(ValueError, match='different n_theta'):
        plain.compare(_solution(n_t=3))
    with pytest.raises(ValueError, match='n_theta = 17 > 16'):
        _solution(n_t=17).compare(_solution(n_t=17))
    with pytest.raises(ValueError, match='more than 256 rows'):
        plain.compare(_solution(rows=257))
    flagged = _solution()
    flagged.is_overlapping = True
    with pytest.raises(ValueError, match=r'remove_overlaps\(\)'):
        plain.compare(flagged)
    with pytest.raises(ValueError, match=r'remove_overlaps\(\)'):
        flagged.compare(plain)
    with pytest.raises(ValueError, match='name the rows to compare'):
        plain.compare(_solution(n_x=3))                       # all rows, but 4 against 3
    with pytest.raises(ValueError, match='row indices of x in 0..3'):
        plain.compare(plain, outputs=[4])
    with pytest.raises(ValueError, match='non-empty'):
        plain.compare(plain, outputs=[])
    with pytest.raises(ValueError, match='tol must be finite'):
        plain.compare(plain, tol=-1.0)
    with pytest.raises(ValueError, match='tol must be finite'):
        plain.compare(plain, tol=numpy.nan)


def test_law_gap_pairs_refuses_before_any_launch(no_device):
    polys, laws, _ = cases.open_half_strip()
    off, ef = cases.csr(polys)
    with pytest.raises(ValueError, match='laws must be'):
        cmp.law_gap_pairs(off, ef, laws[:2], [0], [1])
    with pytest.raises(ValueError, match='outside 1..256'):
        cmp.law_gap_pairs(off, ef, numpy.zeros((3, 257, 3)), [0], [1])
    with pytest.raises(ValueError, match='index arrays'):
        cmp.law_gap_pairs(off, ef, laws, [0], [3])
    with pytest.raises(ValueError, match='index arrays'):
        cmp.law_gap_pairs(off, ef, laws, [0, 1], [1])
    with pytest.raises(ValueError, match='tol must be finite'):
        cmp.law_gap_pairs(off, ef, laws, [0], [1], tol=numpy.inf)
    with pytest.raises(ValueError, match='rows and laws must be finite'):
        cmp.law_gap_pairs(off, ef, numpy.where(laws == 1.0, numpy.nan, laws), [0], [1])
    with pytest.raises(ValueError, match='xs must be'):
        cmp.law_gap_pairs(off, ef, laws, [0], [1], xs=numpy.zeros((2, 2)))
    with pytest.raises(ValueError, match='1..256 rows'):
        cmp.law_gap_pairs(numpy.array([0, 257, 258, 259]), numpy.tile(ef[:1], (259, 1)), laws, [0], [1])
    res = cmp.law_gap_pairs(off, ef, laws, [], [], ranges=True)            # no pairs: no launch
    assert len(res['gap']) == 0 and res['ranges'].shape == (0, 1, 2) and res['stats']['pairs'] == 0
