"""The references of tests/test_gpu_locate.py checked on their own: the exactness claim of the lattice data (recomputed with
fractions.Fraction), the thermometer-grid generator, the share of points the wide reference leaves out, and the facet LP."""
from fractions import Fraction

import numpy
import pytest

import locate_reference as ref
from locate_reference import LATTICE, TOL


def _fraction_scan(row_off, ef, xlaw, theta, tol, overlapping, inclusive, Q, c, H):
    """the contract for one point in exact rational arithmetic: (region, x or None)"""
    F = Fraction
    th = [F(float(v)) for v in theta]
    found, best = -1, None
    for r in range(len(row_off) - 1):
        rows = ef[row_off[r]:row_off[r + 1]]
        if len(rows) == 0:
            continue
        inside = True
        for row in rows:
            v = sum(F(float(e)) * t for e, t in zip(row[1:], th))
            inside = inside and (v <= F(float(row[0])) + F(tol) if inclusive else v - F(float(row[0])) < F(tol))
        if not inside:
            continue
        if not overlapping:
            found = r
            break
        x = [F(float(l[0])) + sum(F(float(a)) * t for a, t in zip(l[1:], th)) for l in xlaw[r]]
        obj = F(0)
        for a in range(len(x)):
            g = F(float(c[a])) if c is not None else F(0)
            if H is not None:
                g += sum(F(float(h)) * t for h, t in zip(H[a], th))
            if Q is not None:
                g += F(1, 2) * sum(F(float(q)) * xj for q, xj in zip(Q[a], x))
            obj += g * x[a]
        if best is None or obj <= best:
            best, found = obj, r
    if found < 0:
        return -1, None
    return found, [F(float(l[0])) + sum(F(float(a)) * t for a, t in zip(l[1:], th)) for l in xlaw[found]]


@pytest.mark.parametrize('n_t,n_x', [(1, 1), (5, 3), (16, 17)])
def test_lattice_arithmetic_is_exact(n_t, n_x):
    """float64 numpy gives what Fraction gives, for regions and for x bit by bit, and exact_bits certifies it beforehand"""
    for coarse, modes in ((False, [(False, False), (False, True)]), (True, [(True, False), (True, True)])):
        row_off, ef, xlaw, Q, c, H, theta = ref.lattice_case(100 * n_t + n_x, n_t, n_x, coarse)
        for tol in (0.0, TOL):
            bits = ref.exact_bits(ef, xlaw, theta, tol, Q, c, H)
            assert bits[0] <= 53 and bits[1] <= 53
            assert not coarse or bits[2] <= 53
            for overlapping, inclusive in modes:
                reg, x = ref.locate(row_off, ef, xlaw, theta, tol, overlapping, inclusive, Q, c, H)
                assert (reg >= 0).sum() >= 5 and (reg < 0).any()
                for p in range(0, len(theta), 3 if n_x < 17 else 11):
                    want, wx = _fraction_scan(row_off, ef, xlaw, theta[p], tol, overlapping, inclusive, Q, c, H)
                    assert reg[p] == want, (p, overlapping, inclusive)
                    if want >= 0:
                        assert [Fraction(float(v)) for v in x[p]] == wx
                    else:
                        assert numpy.all(numpy.isnan(x[p]))


def test_the_worst_case_of_the_lattice_fits_a_double():
    """multiples of 2^-12 up to 2^8 in 16 dimensions: row tests and x need 46 bits; the objective does not fit in general"""
    ef = numpy.full((1, 17), 256.0 - LATTICE)
    xlaw = numpy.full((1, 17, 17), 256.0 - LATTICE)
    theta = numpy.full((1, 16), 256.0 - LATTICE)
    row, x, obj = ref.exact_bits(ef, xlaw, theta, TOL, Q=numpy.full((17, 17), 256.0 - LATTICE))
    assert row <= 46 and x <= 46 and obj > 53


def test_rules_of_the_contract():
    ef_box = ref.box_rows([-1.0], [1.0])
    row_off, ef = ref.stack([numpy.zeros((0, 2)), ef_box, ef_box, numpy.zeros((0, 2))], 1)
    xlaw = numpy.array([[[9.0, 0.0]], [[1.0, 1.0]], [[1.0, 1.0]], [[7.0, 0.0]]])
    theta = numpy.array([[0.0], [1.0], [1.0 + TOL], [numpy.nan], [5.0]])
    reg, x = ref.locate(row_off, ef, xlaw, theta, TOL)
    assert reg.tolist() == [1, 1, -1, -1, -1]                       # a region without rows holds nothing; strict: tol is outside
    assert x[0, 0] == 1.0 and numpy.isnan(x[2:]).all()
    assert ref.locate(row_off, ef, xlaw, theta, TOL, inclusive=True)[0].tolist() == [1, 1, 1, -1, -1]
    assert ref.locate(row_off, ef, xlaw, theta, TOL, overlapping=True)[0].tolist() == [2, 2, -1, -1, -1]   # a tie goes to the later
    assert ref.locate(row_off, ef, xlaw, theta, 0.0)[0].tolist() == [1, -1, -1, -1, -1]
    assert ref.locate(row_off, ef, xlaw, theta, 0.0, inclusive=True)[0].tolist() == [1, 1, -1, -1, -1]
    assert ref.locate(numpy.zeros(1, dtype=numpy.int64), numpy.zeros((0, 2)), numpy.zeros((0, 1, 2)), theta, TOL)[0].tolist() == [-1] * 5


@pytest.mark.parametrize('shape', sorted(ref.WIDE_CASES))
def test_wide_cases_leave_out_at_most_one_percent(shape):
    case = ref.wide_case(shape)
    assert len(case['theta']) == ref.WIDE_POINTS
    for overlapping, inclusive in ((False, False), (False, True), (True, False)):
        reg, x, keep, xb = ref.locate_wide(case['row_off'], case['ef'], case['xlaw'], case['theta'], case['tol'], overlapping, inclusive,
                                           case['Q'], case['c'], case['H'])
        assert numpy.mean(~keep) <= 0.01
        hit = reg[keep] >= 0
        assert hit.mean() >= 0.2 and (~hit).mean() >= 0.2 and len(numpy.unique(reg[keep])) >= len(case['row_off']) // 2
        assert numpy.all(xb[reg >= 0] > 0)
    # the overlap rule is exercised: it answers differently from the first match on a good share of the points
    first = ref.locate_wide(case['row_off'], case['ef'], case['xlaw'], case['theta'], case['tol'])[0]
    assert numpy.mean(first != reg) >= 0.02


def test_wide_reference_agrees_with_float64_where_it_keeps_a_point():
    """the derived bound is sound against numpy's own float64 evaluation: no kept point changes its region"""
    case = ref.wide_case((8, 24, 20))
    for inclusive in (False, True):
        reg, x, keep, xb = ref.locate_wide(case['row_off'], case['ef'], case['xlaw'], case['theta'], case['tol'], inclusive=inclusive)
        r64, x64 = ref.locate(case['row_off'], case['ef'], case['xlaw'], case['theta'], case['tol'], inclusive=inclusive)
        assert numpy.array_equal(reg[keep], r64[keep])
        ok = keep & (reg >= 0)
        assert numpy.all(numpy.abs(x64[ok] - x[ok].astype(float)) <= xb[ok])


@pytest.mark.parametrize('name', sorted(ref.GRIDS))
def test_thermometer_grid_generator(name):
    g = ref.GRIDS[name]()
    cells = g.shuffled(3)
    assert sorted(cells) == g.all_cells() and cells != g.all_cells()
    b = g.build(cells)
    index = {cell: i for i, cell in enumerate(cells)}
    masks = [tuple(int(w) for w in row) for row in b['masks']]
    assert len(set(masks)) == len(masks)
    assert numpy.all(b['ef'] / LATTICE == numpy.rint(b['ef'] / LATTICE)) and numpy.max(numpy.abs(b['ef'])) <= 256
    by_mask = {m: i for i, m in enumerate(masks)}
    seen_words = set()
    for i, cell in enumerate(cells):
        rows = b['ef'][b['row_off'][i]:b['row_off'][i + 1]]
        info = b['row_info'][b['row_off'][i]:b['row_off'][i + 1]]
        assert len(rows) == 2 * g.n_t
        centre = g.centre(cell)
        assert numpy.all(rows[:, 1:] @ centre - rows[:, 0] < -10 * TOL)
        for k, (row, inf) in enumerate(zip(rows, info)):
            kind, ident = int(inf) >> 16, int(inf) & 0xffff
            a, upper = k // 2, k % 2 == 0
            assert row[1 + a] == (1.0 if upper else -1.0) and numpy.count_nonzero(row[1:]) == 1
            if kind == ref.KIND_OMEGA:
                assert row[0] == g.outer if a not in g.axes else row[0] in (g.cuts[a][-1], -g.cuts[a][0])
                continue
            assert kind == (ref.KIND_INACTIVE if upper else ref.KIND_LAMBDA)
            assert (ident in g.active_set(cell)) == (kind == ref.KIND_LAMBDA)
            seen_words.add(ident >> 6)
            key = list(masks[i])
            key[ident >> 6] ^= 1 << (ident & 63)
            j = by_mask[tuple(key)]                      # the cell behind the row exists ...
            step = tuple(c + ((1 if upper else -1) if ax == a else 0) for ax, c in zip(g.axes, cell))
            assert cells[j] == step                      # ... and is the one on the other side of the cut
            other = b['ef'][b['row_off'][j]:b['row_off'][j + 1]]
            assert numpy.array_equal(other[k + 1 if upper else k - 1], -row)
    assert len(seen_words) >= 2                          # the ids cross a word edge of the masks
    if g.mask_words == 4:
        assert seen_words <= {1, 2, 3} and {2, 3} <= seen_words


def test_the_issue_example_is_a_corner_case_for_the_reference():
    """3 x 2 boxes, cuts theta_1 in {-2, 0}, theta_2 = 0: the point (-tol/2, -tol/2) lies in A strictly and in D within tol"""
    g = ref.Grid(2, {0: [-4.0, -2.0, 0.0, 4.0], 1: [-4.0, 0.0, 4.0]}, {0: 0, 1: 70}, 128, 2)
    cells = [(0, 0), (2, 1), (1, 0), (2, 0), (1, 1), (0, 1)]
    b = g.build(cells)
    p = numpy.array([[-TOL / 2, -TOL / 2]])
    laws = numpy.zeros((6, 1, 3))
    assert ref.locate(b['row_off'], b['ef'], laws, p, TOL)[0].tolist() == [1]
    assert ref.locate(b['row_off'], b['ef'], laws, p, 0.0)[0].tolist() == [2]


def test_facet_reference_on_closed_forms():
    for n in (1, 2, 5):
        rng = numpy.random.default_rng(n)
        sides = rng.integers(1, 9, size=n) * 0.25
        lo = rng.integers(-8, 8, size=n) * 0.5
        st, ce, ra = ref.facet_centres(*ref.stack([ref.box_rows(lo, lo + sides)], n))
        assert numpy.all(st == ref.LP_OPTIMAL)
        assert numpy.allclose(ra, [ref.box_facet_radius(sides, k // 2) for k in range(2 * n)], rtol=0, atol=1e-9)
        st, ce, ra = ref.facet_centres(*ref.stack([ref.simplex_rows(n)], n))
        assert numpy.all(st == ref.LP_OPTIMAL) and numpy.allclose(ra, ref.simplex_radii(n), rtol=0, atol=1e-9)
    # a strictly redundant row; a wedge whose facets go to infinity; the half-strip {theta_1 >= 0, |theta_2| <= 1}, whose long facets are
    # unbounded sets but whose LP is bounded by the opposite row (radius 2; the end facet has radius 1)
    redundant = numpy.vstack([ref.box_rows([-1.0, -1.0], [1.0, 1.0]), [[5.0, 1.0, 0.0]]])
    assert ref.facet_centre(redundant, 4)[0] == ref.LP_INFEASIBLE
    wedge = numpy.array([[0.0, -1.0, 0.0], [1.0, 0.0, 1.0]])
    assert [ref.facet_centre(wedge, q)[0] for q in range(2)] == [ref.LP_UNBOUNDED] * 2
    strip = numpy.array([[0.0, -1.0, 0.0], [1.0, 0.0, 1.0], [1.0, 0.0, -1.0]])
    got = [ref.facet_centre(strip, q) for q in range(3)]
    assert [s for s, _, _ in got] == [ref.LP_OPTIMAL] * 3 and numpy.allclose([r for _, _, r in got], [1.0, 2.0, 2.0], atol=1e-9)
    for q, (s, cen, r) in enumerate(got):
        assert ref.certificate_violation(strip, q, cen, r) <= ref.LP_TOL


def test_tangent_polytopes_have_only_clear_facets():
    """every row of the random polytopes of the facet tests is a facet with a radius far above the LP tolerance"""
    for n, m, seed in ref.FACET_SHAPES:
        rows = ref.tangent_polytope(numpy.random.default_rng(seed), n, m)
        st, ce, ra = ref.facet_centres(*ref.stack([rows], n))
        assert numpy.all(st == ref.LP_OPTIMAL) and ra.min() > 1e-6, (n, m, ra.min())
        assert max(ref.certificate_violation(rows, q, ce[q], ra[q]) for q in range(m)) <= ref.LP_TOL

