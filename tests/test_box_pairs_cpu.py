"""The rule of the candidate sweep and of the row screen, without a device: the numpy reference of box_pairs_reference.py
against the three host sweeps on boxes that decide every pair exactly, the corner cases in which the host sweeps differ from the rule,
the Python-side refusals of the new wrappers and arguments, and the safety of the screen on the BSP sets of compare_cases.py."""
import functools
import sys

import numpy
import pytest
from scipy.optimize import linprog

import box_pairs_reference as ref
import compare_cases as cases
from ppopt_amd import _lib, compare, overlap, transition
from ppopt_amd.geometry import box_pairs as bp_module      # noqa: F401  (ppopt_amd.geometry exports the function under the module's name)

bp = sys.modules['ppopt_amd.geometry.box_pairs']

TOL = ref.TOL
INF, NAN = numpy.inf, numpy.nan
SIZES = [(1, 1), (65, 63), (257, 130)]


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype == numpy.int64 and numpy.array_equal(g, w)


# ---- 1. boxes that decide every pair exactly ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_t', [1, 2, 5, 16])
@pytest.mark.parametrize('ra,rb', SIZES)
def test_reference_equals_the_host_sweeps_on_dyadic_boxes(n_t, ra, rb):
    a, b = ref.dyadic_boxes(ra, n_t, 10 * n_t + 1), ref.dyadic_boxes(rb, n_t, 10 * n_t + 2)
    ua, ub = numpy.arange(ra) % 7 != 3, numpy.arange(rb) % 5 != 1
    # every difference of two bounds is exact: bounds are multiples of 2^-10 below 8
    for box in (a, b):
        assert numpy.all(box * 1024 == numpy.round(box * 1024)) and numpy.abs(box).max() < 8
    _same(compare.cross_box_pairs(a, ua, b, ub, TOL), ref.all_pairs(a, ua, b, ub, TOL))
    _same(overlap.box_pairs(a, ua, TOL), ref.all_pairs(a, ua, margin=TOL))
    # the transition graph: image boxes against region boxes of the same regions, margin -tol, i = j included
    c = ref.dyadic_boxes(ra, n_t, 10 * n_t + 3)
    got = transition.image_box_pairs(a, c, ua, TOL)
    _same(got, ref.all_pairs(a, ua, c, ua, -TOL))
    if ra > 1:
        # the strict compare is pinned: pairs that overlap by exactly the margin exist, and are not listed
        assert ref.exact_ties(a, b, TOL) > ra and ref.exact_ties(a, c, -TOL) > ra
        assert len(ref.all_pairs(a, ua, b, ub, TOL)[0]) > 0 and len(got[0]) > 0


def test_the_strict_compare_by_hand():
    a = numpy.array([[[0.0], [1.0]]])
    b = numpy.array([[[1.0 - TOL], [2.0]], [[1.0 - 2 * TOL], [2.0]], [[1.0 + TOL], [2.0]], [[1.0 + TOL / 2], [2.0]]])
    one, all4 = numpy.ones(1, dtype=bool), numpy.ones(4, dtype=bool)
    assert ref.all_pairs(a, one, b, all4, TOL)[1].tolist() == [1]             # an overlap of exactly tol is none
    assert ref.all_pairs(a, one, b, all4, -TOL)[1].tolist() == [0, 1, 3]      # a gap of exactly tol is none
    _same(compare.cross_box_pairs(a, one, b, all4, TOL), ref.all_pairs(a, one, b, all4, TOL))


# ---- 2. corner cases: where the host sweeps differ from the rule --------------------------------------------------------------------------
def test_corner_cases_and_what_the_host_sweeps_do_with_them():
    """The finding of DESIGN §3.27:
      NaN bound   the rule opens that bound alone.  cross_box_pairs does the same.  overlap.box_pairs opens nothing: a box with a NaN
                  meets no box.  image_box_pairs opens BOTH bounds of the coordinate.
      inf - inf   fails the rule, in cross_box_pairs and in overlap.box_pairs.  image_box_pairs keeps a pair whose difference is NaN in a
                  coordinate other than the first (its sweep along the first coordinate drops it there).
      infinite bounds and the whole-space box are ordinary everywhere."""
    whole = [[-INF, -INF], [INF, INF]]
    fam = numpy.array([[[0.0, 0.0], [1.0, 1.0]],          # 0 the unit square
                       whole,                              # 1 the whole space
                       [[2.0, -INF], [INF, 0.5]],          # 2 a quadrant-like box right of the square
                       [[0.5, 0.5], [NAN, 0.75]],          # 3 NaN upper bound: open to the right
                       [[NAN, 3.0], [0.25, 4.0]],          # 4 NaN lower bound: open to the left, above the square
                       [[0.5, INF], [0.75, INF]],          # 5 lower = upper = +inf in coordinate 1
                       [[0.5, 0.25], [NAN, 0.75]]])        # 6 NaN upper bound again
    use = numpy.ones(len(fam), dtype=bool)
    tol = TOL
    # the rule, by hand: 5 meets nothing whose upper bound is +inf in coordinate 1 (inf - inf), and nothing else either
    want_cross = {(0, 0), (0, 1), (0, 3), (0, 6), (1, 1), (1, 2), (1, 3), (1, 4), (1, 6), (2, 2), (2, 6), (3, 3), (3, 6), (4, 4), (6, 6)}
    want_cross |= {(j, i) for i, j in want_cross}
    got = ref.all_pairs(fam, use, fam, use, tol)
    assert set(zip(got[0].tolist(), got[1].tolist())) == want_cross
    up = ref.all_pairs(fam, use, margin=tol)
    assert set(zip(up[0].tolist(), up[1].tolist())) == {(i, j) for i, j in want_cross if i < j}
    assert (1, 5) not in want_cross and (5, 5) not in want_cross           # inf - inf fails, against the whole space and against itself
    # cross_box_pairs: the rule
    _same(compare.cross_box_pairs(fam, use, fam, use, tol), got)
    # overlap.box_pairs: a NaN drops the box; the rule with the NaN boxes masked
    nan_box = numpy.isnan(fam).any(axis=(1, 2))
    assert nan_box.tolist() == [False, False, False, True, True, False, True]
    host = overlap.box_pairs(fam, use, tol)
    assert set(zip(host[0].tolist(), host[1].tolist())) == {(0, 1), (1, 2)} != set(zip(up[0].tolist(), up[1].tolist()))
    _same(host, ref.all_pairs(fam, use & ~nan_box, margin=tol))
    # image_box_pairs: both bounds of a NaN coordinate open (3 then meets 4 and 2 in coordinate 0 whatever its lower bound), and the NaN
    # difference of 5 against the whole space in coordinate 1 is kept
    host = transition.image_box_pairs(fam, fam, use, tol)
    rule = ref.all_pairs(fam, use, fam, use, -tol)
    host_set, rule_set = set(zip(host[0].tolist(), host[1].tolist())), set(zip(rule[0].tolist(), rule[1].tolist()))
    assert (1, 5) in host_set and (5, 1) in host_set and (5, 5) in host_set and (1, 5) not in rule_set
    patched = fam.copy()
    unknown = numpy.isnan(fam).any(axis=1)
    patched[:, 0][unknown], patched[:, 1][unknown] = -INF, INF
    fixed = ref.all_pairs(patched, use, patched, use, -tol)
    # with the NaN coordinates opened first, the rule and image_box_pairs differ in the inf - inf pairs alone
    assert host_set - set(zip(fixed[0].tolist(), fixed[1].tolist())) == {(1, 5), (5, 1), (5, 5)}
    assert set(zip(fixed[0].tolist(), fixed[1].tolist())) <= host_set
    # without box 5 (a box no kernel produces: DESIGN §3.27) the patched rule IS image_box_pairs
    use5 = use.copy()
    use5[5] = False
    _same(transition.image_box_pairs(fam, fam, use5, tol), ref.all_pairs(patched, use5, patched, use5, -tol))


def test_the_image_box_is_widened_before_rows_screen_it():
    """what the complete config 3 showed: the flat image of a region under a singular map lies in the facet theta_0 <= 5 of its
    target, and its computed upper bound is 5 + 6.1e-12.  The raw box is separated by that row, by a hair; the box the screen is given
    (transition.screen_box) is not, and still is by every row that is more than 1e-7 away."""
    image = numpy.array([[[5.0 + 6.1e-12, -1.0], [5.0 + 6.1e-12, 1.0]], [[-INF, NAN], [INF, 0.5]]])
    target = numpy.array([[5.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    far = numpy.array([[5.0 - 1e-7, 1.0, 0.0]])
    assert ref.row_separates(target[0], image[0]) and not ref.row_separates(target[1], image[0])
    outer = transition.screen_box(image, 1e-8)
    assert not any(ref.row_separates(r, outer[0]) for r in target) and ref.row_separates(far[0], outer[0])
    assert numpy.all(outer[0, 0] < image[0, 0]) and numpy.all(outer[0, 1] > image[0, 1])
    assert numpy.all(numpy.abs(outer[0] - image[0]) <= 1e-8 * (1.0 + numpy.abs(image[0])) * (1 + 1e-6))
    assert outer[1, 0, 0] == -INF and outer[1, 1, 0] == INF and numpy.isnan(outer[1, 0, 1]) and outer[1, 1, 1] > 0.5
    assert numpy.array_equal(transition.screen_box(image, 0.0)[0, 1], image[0, 1] + 1e-9 * (1.0 + numpy.abs(image[0, 1])))      # tol = 0: the floor


# ---- 3. refusals on the Python side: ValueError, and the library is never loaded ----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', refuse)


def test_python_side_refusals_of_the_wrappers(no_library):
    box, use = ref.dyadic_boxes(5, 2, 0), numpy.ones(5, dtype=bool)
    for kw, text in ((dict(box_a=box[:, 0], usable_a=use), r'\[R, 2, n_t\]'), (dict(box_a=box[:0], usable_a=use[:0]), 'holds no box'),
                     (dict(box_a=numpy.zeros((5, 2, 17)), usable_a=use), r'outside 1\.\.16'), (dict(box_a=box, usable_a=use[:4]), 'one usable entry'),
                     (dict(box_a=box, usable_a=None), 'usable'), (dict(box_a=box, usable_a=use, usable_b=use), 'usable_b without box_b'),
                     (dict(box_a=box, usable_a=use, box_b=numpy.zeros((5, 2, 3)), usable_b=use), 'different n_theta'),
                     (dict(box_a=box, usable_a=use, box_b=box[:0], usable_b=use[:0]), 'holds no box'),
                     (dict(box_a=box, usable_a=use, margin=numpy.nan), 'margin must be finite'), (dict(box_a=box, usable_a=use, margin=INF), 'margin must be finite'),
                     (dict(box_a=box, usable_a=use, rows=(2, 6)), 'rows'), (dict(box_a=box, usable_a=use, rows=(3, 2)), 'rows'),
                     (dict(box_a=box, usable_a=use, rows=(-1, 2)), 'rows'), (dict(box_a=box, usable_a=use, cap=-1), 'cap must be >= 0')):
        with pytest.raises(ValueError, match=text):
            bp.box_pairs(**kw)
    polys = [ref.axis_rows(b) for b in box]
    off, ef = cases.csr(polys)
    ok = dict(row_off=off, ef_rows=ef, pair_a=[0, 1], pair_b=[1, 2], box_for_a_rows=box, box_for_b_rows=box)
    for kw, text in ((dict(sides='c'), 'sides'), (dict(pair_a=[0, 5]), 'index arrays'), (dict(pair_b=[-1, 0]), 'index arrays'), (dict(pair_a=[0]), 'index arrays'),
                     (dict(box_for_a_rows=None), 'needs box_for_a_rows'), (dict(box_for_b_rows=None, sides='b'), 'needs box_for_b_rows'),
                     (dict(box_for_b_rows=box[:4]), r'must be \[5, 2, 2\]'), (dict(row_off=off[:-1]), 'row_off'),
                     (dict(ef_rows=numpy.zeros((len(ef), 18))), r'outside 1\.\.16')):
        with pytest.raises(ValueError, match=text):
            bp.screen_pairs(**dict(ok, **kw))
    keep, stats = bp.screen_pairs(**dict(ok, pair_a=[], pair_b=[]))       # no candidate: no call
    assert keep.dtype == bool and len(keep) == 0 and stats['pairs'] == 0
    assert bp.screen_pairs(**dict(ok, pair_a=[], pair_b=[], box_for_a_rows=None, sides='b'))[1]['dropped'] == 0


def test_sweep_and_screen_arguments_are_checked_before_anything_else(no_library):
    for who in ('compare', 'transition_graph'):
        for kw in (dict(sweep='gpu'), dict(screen='boxes'), dict(sweep=None), dict(screen=True)):
            with pytest.raises(ValueError, match='sweep must be|screen must be'):
                bp.sweep_options(who, **dict(dict(sweep='host', screen='none'), **kw))
    assert bp.sweep_options('x', 'host', 'none') == (False, False) and bp.sweep_options('x', 'device', 'rows') == (True, True)
    polys = [ref.axis_rows(b) for b in ref.dyadic_boxes(3, 2, 1)]
    off, ef = cases.csr(polys)
    with pytest.raises(ValueError, match="sweep must be 'host' or 'device'"):
        transition.transition_pairs(off, ef, numpy.zeros((3, 2, 2)), numpy.zeros((3, 2)), 2, sweep='both')
    with pytest.raises(ValueError, match="screen must be 'none' or 'rows'"):
        overlap.partition_by_value(off, ef, numpy.zeros((3, 2)), numpy.zeros(3), 2, screen='row')
    # the public calls refuse before they look at the solution: no solution is needed to see it
    with pytest.raises(ValueError, match='sweep must be'):
        compare.compare_solutions(None, None, sweep='Device')
    with pytest.raises(ValueError, match='screen must be'):
        transition.transition_graph(None, None, None, None, screen='all')
    with pytest.raises(ValueError, match='sweep must be'):
        overlap.remove_overlaps(None, sweep='')
    from ppopt_amd import Solution
    import inspect
    for name in ('compare', 'transition_graph', 'remove_overlaps'):
        p = inspect.signature(getattr(Solution, name)).parameters
        assert p['sweep'].default == 'host' and p['screen'].default == 'none'


# ---- 4. the screen never drops a pair whose intersection has a point ------------------------------------------------------------------------
def _lp_box(poly):
    """[2, n] the bounding box of a bounded polytope by 2 n LPs, widened by 1e-9: the screen's argument needs a box that CONTAINS the set,
    and an LP solver's optimum is accurate to its feasibility tolerance only"""
    n = poly.shape[1] - 1
    out = numpy.zeros((2, n))
    for k in range(n):
        for side, sign in ((0, 1.0), (1, -1.0)):
            r = linprog(sign * numpy.eye(n)[k], A_ub=poly[:, 1:], b_ub=poly[:, 0], bounds=[(None, None)] * n, method='highs-ds')
            assert r.status == 0
            out[side, k] = sign * r.fun - sign * 1e-9
    return out


def _has_a_point(rows):
    n = rows.shape[1] - 1
    r = linprog(numpy.zeros(n), A_ub=rows[:, 1:], b_ub=rows[:, 0], bounds=[(None, None)] * n, method='highs-ds')
    assert r.status in (0, 2)
    return r.status == 0


@functools.lru_cache(maxsize=None)
def bsp_screen_case(n):
    """(polys, boxes [R, 2, n], n_a, pair_a, pair_b (table indices), feasible [pairs]) of synthetic(n): EVERY pair (A cell, B cell)"""
    polys, _, n_a = cases.table(cases.synthetic(n))
    boxes = numpy.stack([_lp_box(p) for p in polys])
    i, j = numpy.divmod(numpy.arange(n_a * (len(polys) - n_a)), len(polys) - n_a)
    j = j + n_a
    feasible = numpy.array([_has_a_point(numpy.vstack([polys[p], polys[q]])) for p, q in zip(i.tolist(), j.tolist())])
    return polys, boxes, n_a, i, j, feasible


@pytest.mark.parametrize('n', [1, 2, 3, 5])
def test_the_screen_reference_never_drops_a_pair_with_a_common_point(n):
    polys, boxes, n_a, i, j, feasible = bsp_screen_case(n)
    assert len(i) == n_a * (len(polys) - n_a) and feasible.sum() >= cases.SHAPES[n][3]      # no pair is left out
    dropped = {}
    for sides in ('a', 'b', 'both'):
        keep = ref.screen(polys, i, j, boxes, boxes, sides)
        assert numpy.all(keep[feasible]), (sides, numpy.flatnonzero(feasible & ~keep))
        dropped[sides] = int((~keep).sum())
    assert dropped['both'] >= max(dropped['a'], dropped['b'])
    if n <= 3:      # and it does drop pairs (at n = 5 the boxes of 16 cells are nearly the whole cube and the screen has nothing to drop)
        assert dropped['both'] > 0
