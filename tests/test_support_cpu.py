"""The host side of the support functions (ppopt_amd/geometry/support.py) and the CPU reference of their device part; no
device: where the library would be called, _lib.support_rows is replaced by the reference."""
import sys

import numpy
import pytest

import reduce_cases as rc
import reduce_reference as rr
import support_cases as sc
import support_reference as ref
from exit_cases import box_rows, csr
from ppopt_amd import Solution, _lib
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.geometry import Polytope, containment, pontryagin_difference, support, support_of

S = sys.modules['ppopt_amd.geometry.support']      # the module: ppopt_amd.geometry.support is the function of that name

TOL = 1e-8


def _poly(rows):
    rows = numpy.asarray(rows, dtype=float)
    return Polytope(rows[:, 1:].copy(), rows[:, :1].copy())


# ---- the reference against closed forms ------------------------------------------------------------------------------------------------
def test_reference_closed_forms():
    sq = box_rows([0, 0], [1, 1])
    for d, want in (([1, 0], 1.0), ([-1, -1], 0.0), ([300, 400], 700.0), ([1e-3, -2e-3], 1e-3)):
        st, v, x = ref.support(sq, d)
        assert st == ref.OPTIMAL and abs(v - want) <= 1e-12 * (1 + abs(want)) and numpy.all(sq[:, 1:] @ x <= sq[:, 0] + 1e-12)
    simplex = numpy.vstack([[0.0, -1, 0, 0], [0.0, 0, -1, 0], [0.0, 0, 0, -1], numpy.append(1.0, numpy.ones(3)) / numpy.sqrt(3.0)])
    assert abs(ref.support(simplex, [1.0, 2.0, 3.0])[1] - 3.0) <= 1e-12 and abs(ref.support(simplex, [-1.0, -2.0, -3.0])[1]) <= 1e-12
    half = numpy.array([[1.0, 1.0, 0.0]])
    assert ref.support(half, [0.0, 1.0])[:2] == (ref.UNBOUNDED, numpy.inf) and ref.support(half, [-1.0, 0.0])[0] == ref.UNBOUNDED
    assert abs(ref.support(half, [2.0, 0.0])[1] - 2.0) <= 1e-12
    twice = numpy.vstack([sq, sq[0]])
    assert abs(ref.support(twice, [1.0, 0.0])[1] - 1.0) <= 1e-12
    assert ref.radius(half)[0] is True and abs(ref.radius(sq)[1] - 0.5) <= 1e-12 and abs(ref.radius(box_rows([0, 0], [0, 1]))[1]) <= 1e-12
    # box - box = box
    empty, rows = ref.erosion(box_rows([-1, -2], [3, 4]), box_rows([-0.25, -0.5], [0.5, 0.125]))
    assert not empty and numpy.allclose(rows, box_rows([-0.75, -1.5], [2.5, 3.875]), atol=1e-12)
    assert ref.erosion(sq, half)[0] is True
    ex, row, x = ref.containment(box_rows([0.25, 0.25], [0.5, 1.25]), sq)
    assert abs(ex - 0.25) <= 1e-12 and row == 1 and abs(x[1] - 1.25) <= 1e-12
    assert ref.containment(half, sq)[0] == numpy.inf


def test_reference_hand_cases_and_no_thin_seeded_set():
    for name, rows, d, want, status in sc.hand_cases():
        thin = not ref.radius(rows)[0] and not ref.radius(rows)[1] > TOL
        assert thin == (name == 'strip')
        for dk, wk, sk in zip(d, want, status):
            if thin or not numpy.any(dk):
                continue
            st, v, _ = ref.support(rows, dk)
            assert (st == ref.UNBOUNDED) == (sk == 1) and (v == wk if sk == 1 else abs(v - wk) <= 1e-12 * (1 + abs(wk))), (name, dk)
    for case in sc.CASES:
        polys, dirs = sc.seeded(case)
        assert [len(d) for d in dirs][:5] == ([200] if case in sc.SINGLES else list(sc.COUNTS)[:len(polys)])
        for p, d in zip(polys, dirs):
            unbounded, r, _ = ref.radius(p)
            assert r > 1e-3 and numpy.all(numpy.isfinite(d)) and d.shape[1] == p.shape[1] - 1


# ---- _lib.support_rows replaced by the reference -----------------------------------------------------------------------------------------
def _fake_support_rows(calls):
    def fake(off, ef, doff, d, start, tol, args=True, device=0):
        calls.append((numpy.array(off), numpy.array(ef), numpy.array(doff), numpy.array(d)))
        n, n_t = len(off) - 1, ef.shape[1] - 1
        value, arg, ds = numpy.zeros(len(d)), numpy.zeros((len(d), n_t)), numpy.zeros(len(d), dtype=numpy.int32)
        ps, wide, point = numpy.zeros(n, dtype=numpy.int32), numpy.zeros(n, dtype=numpy.int32), numpy.zeros((n, n_t))
        stats = dict(polytopes=n, thin=0, directions=len(d), zero=0, lps=n, pivots=0, wide=0, ms=0.0)
        for q in range(n):
            rows = ef[off[q]:off[q + 1]]
            unbounded, r, point[q] = ref.radius(rows)
            thin = not unbounded and not r > tol
            ps[q] = S.THIN if thin else S.OK
            stats['thin'] += int(thin)
            for g in range(doff[q], doff[q + 1]):
                if thin:
                    value[g], arg[g], ds[g] = numpy.nan, numpy.nan, S.THIN
                elif not numpy.any(d[g] != 0.0):
                    arg[g] = point[q]
                    stats['zero'] += 1
                else:
                    st, v, x = ref.support(rows, d[g])
                    stats['lps'] += 1
                    value[g], ds[g] = v, (S.UNBOUNDED if st == ref.UNBOUNDED else S.OK)
                    arg[g] = point[q] if x is None else x
                    stats['wide'] += int(st == ref.UNBOUNDED)
        return value, (arg if args else None), ds, ps, wide, point, stats
    return fake


@pytest.fixture
def calls(monkeypatch):
    made = []
    monkeypatch.setattr(_lib, 'support_rows', _fake_support_rows(made))
    return made


def test_symbol_and_constants():
    assert 'mpc_support_rows' in _lib.EXPORTED_SYMBOLS
    assert (_lib.SUPPORT_OK, _lib.SUPPORT_UNBOUNDED, _lib.SUPPORT_CAPPED, _lib.SUPPORT_THIN) == (0, 1, 2, 3) == (S.OK, S.UNBOUNDED, S.CAPPED, S.THIN)
    assert _lib.SUPPORT_MAX_ROWS == S.MAX_ROWS == 512


def test_support_csr_plumbing(calls):
    cases = [c for c in sc.hand_cases() if c[1].shape[1] == 3]
    off, ef = csr([c[1] for c in cases])
    doff, d = csr([c[2] for c in cases])
    r = support_of(off, ef, 2, doff, d, tol=TOL)
    assert len(calls) == 1 and calls[0][2].tolist() == doff.tolist() and calls[0][3].tobytes() == d.tobytes()
    for q, c in enumerate(cases):
        got = r.values_of(q)
        assert len(got) == len(c[2]) and r.dir_status[doff[q]:doff[q + 1]].tolist() == c[4]
        for g, w in zip(got, c[3]):
            assert numpy.isnan(g) if w is None else (g == w if numpy.isinf(w) else abs(g - w) <= 1e-12 * (1 + abs(w)))
    assert r.poly_status.tolist() == [0, 0, 0, 3, 0, 0] and r.stats['directions'] == 27 and r.stats['zero'] == 2 and r.stats['thin'] == 1
    assert 'device_ms' in r.stats and 'wall_ms' in r.stats
    # Polytope objects: one array for all, a list with one array each, rows of any length
    sq = _poly(box_rows([0, 0], [1, 1]) * 3.0)
    r = support([sq, sq], numpy.array([[1.0, 1.0]]))
    assert r.dir_off.tolist() == [0, 1, 2] and numpy.allclose(r.value, 2.0, atol=1e-12) and numpy.allclose(calls[-1][1], numpy.tile(box_rows([0, 0], [1, 1]), (2, 1)))
    r = support([sq, sq], [numpy.zeros((0, 2)), numpy.array([[1.0, 0.0], [0.0, -2.0]])])
    assert r.dir_off.tolist() == [0, 0, 2] and numpy.allclose(r.value, [1.0, 0.0], atol=1e-12)
    v, a = sq.support([[2.0, 2.0]])
    assert numpy.allclose(v, [4.0]) and numpy.allclose(a, [[1.0, 1.0]])
    v, a = sq.support([0.0, -1.0])
    assert abs(v) <= 1e-12 and a.shape == (2,)


def test_pontryagin_difference_dedupe_scatter_and_map(calls):
    P = [_poly(box_rows([-1, -2], [3, 4])), _poly(box_rows([0, 0], [2, 2]) * 2.0)]
    Q = _poly(box_rows([-0.25, -0.5], [0.5, 0.125]))
    r = pontryagin_difference(P, Q, reduce_rows=False)
    # the two boxes share their four normals: four distinct directions go out once, eight values come back
    assert len(calls) == 1 and len(calls[0][3]) == 4 and calls[0][2].tolist() == [0, 4] and r.stats['directions'] == 4
    assert r.status.tolist() == [S.ERODED_OK] * 2 and r.row_off.tolist() == [0, 4, 8] and len(r.support) == 8
    assert numpy.allclose(r.rows_of(0), box_rows([-0.75, -1.5], [2.5, 3.875]), atol=1e-12)
    assert numpy.allclose(r.rows_of(1), box_rows([0.25, 0.5], [1.5, 1.875]), atol=1e-12)
    unit = numpy.vstack([box_rows([-1, -2], [3, 4]), box_rows([0, 0], [2, 2])])
    assert r.rows[:, 1:].tobytes() == unit[:, 1:].tobytes() and r.rows[:, 0].tobytes() == (unit[:, 0] - r.support).tobytes()
    # one Q per P: no dedupe, the directions in row order
    per = pontryagin_difference(P, [Q, Q], reduce_rows=False)
    assert len(calls[-1][3]) == 8 and calls[-1][2].tolist() == [0, 4, 8] and per.rows.tobytes() == r.rows.tobytes()
    # E' n: a 1-D disturbance w in [-1, 1] entering through E = (0.5, 0.25)': h = |E' n|
    E = numpy.array([[0.5], [0.25]])
    W = _poly(numpy.array([[1.0, 1.0], [1.0, -1.0]]))
    r = pontryagin_difference(P[0], W, E=E, reduce_rows=False)
    assert calls[-1][3].shape[1] == 1 and sorted(calls[-1][3].reshape(-1).tolist()) == [-0.5, -0.25, 0.25, 0.5]
    assert numpy.allclose(r.rows_of(0), box_rows([-0.5, -1.75], [2.5, 3.75]), atol=1e-12)
    assert P[0].erode(W, E=E, reduce_rows=False).A.tobytes() == box_rows([0, 0], [1, 1])[:, 1:].tobytes()


def test_pontryagin_difference_empty_and_thin_q(calls):
    sq = _poly(box_rows([0, 0], [1, 1]))
    half = _poly(numpy.array([[1.0, 1.0, 0.0]]))
    r = pontryagin_difference([sq, half], half, reduce_rows=False)
    # the square asks for h(-x) = +inf; the half-plane itself asks for h(+x) alone
    assert r.status.tolist() == [S.ERODED_EMPTY, S.ERODED_OK] and r.row_off.tolist() == [0, 0, 1] and r.wide.tolist() == [3, 0]
    assert numpy.allclose(r.rows, [[0.0, 1.0, 0.0]]) and len(r.polytopes()[0].A) == 0
    # a Q that does not hold the origin: P - Q moves P the other way; the flag of Q's radius run is carried into wide
    away = _poly(numpy.array([[-1.0, 1.0, 0.0]]))
    real = _lib.support_rows

    def flagged(*a, **kw):
        out = list(real(*a, **kw))
        out[4] = numpy.ones_like(out[4])
        return tuple(out)
    _lib.support_rows = flagged          # the fixture's monkeypatch puts the library's own back
    r = pontryagin_difference(half, away, reduce_rows=False)
    assert r.status.tolist() == [S.ERODED_OK] and numpy.allclose(r.rows, [[2.0, 1.0, 0.0]]) and r.wide.tolist() == [1]
    with pytest.raises(ValueError, match='Polytope.erode: the difference is EMPTY'):
        sq.erode(half)
    with pytest.raises(ValueError, match='Q is THIN'):
        pontryagin_difference(sq, _poly(box_rows([0, 0], [0, 1])))


def test_containment_pair_expansion(calls):
    sq, small, far = box_rows([0, 0], [1, 1]), box_rows([0.25, 0.25], [0.5, 0.75]), box_rows([0.25, 0.25], [0.5, 1.25])
    tri = numpy.vstack([sq[2:], numpy.append(1.0, numpy.ones(2)) / sc.S2])
    inner, outer = [_poly(small), _poly(far)], [_poly(sq), _poly(tri)]
    pairs = [(1, 0), (0, 1), (0, 0), (1, 0)]
    c = containment(inner, outer, pairs=pairs)
    # inner 0 has the rows of its partners 1, 0 in pair order, inner 1 those of 0, 0
    assert calls[0][2].tolist() == [0, 7, 15]
    assert calls[0][3].shape == (15, 2) and numpy.allclose(calls[0][3], numpy.vstack([tri, sq, sq, sq])[:, 1:], rtol=0, atol=1e-15)
    assert c.pairs.tolist() == [list(p) for p in pairs] and c.inside.tolist() == [False, False, True, False]
    assert numpy.allclose(c.excess, [0.25, 0.25 / sc.S2, -0.25, 0.25], atol=1e-12) and c.row.tolist() == [1, 2, 1, 1]
    assert numpy.allclose(c.witness[0][1], 1.25) and numpy.allclose(c.witness[1], [0.5, 0.75])
    for (i, j), ex, row in zip(pairs, c.excess, c.row):
        want = ref.containment([small, far][i], [sq, tri][j])
        assert abs(ex - want[0]) <= 1e-12 and row == want[1]
    both = containment(inner, outer)
    assert both.pairs.tolist() == [[0, 0], [1, 1]] and both.inside.tolist() == [True, False]
    assert _poly(sq).contains_polytope(_poly(small)) and not _poly(small).contains_polytope(_poly(sq))
    half = _poly(numpy.array([[1.0, 1.0, 0.0]]))
    unb = containment(half, _poly(sq))
    assert unb.excess[0] == numpy.inf and not unb.inside[0]
    thin = containment(_poly(box_rows([0, 0], [0, 1])), _poly(sq))
    assert numpy.isnan(thin.excess[0]) and not thin.inside[0] and thin.row[0] == -1


def _solution():
    """two regions over theta in R^2: the square with the law rows (2 theta_0 - theta_1 + 1, 5, -theta_1), the box [1, 3] x [0, 1] with
    rows (theta_0, 7, theta_0 + theta_1); E, f not unit"""
    sq, bx = box_rows([0, 0], [1, 1]), box_rows([1, 0], [3, 1])
    A0, b0 = numpy.array([[2.0, -1.0], [0.0, 0.0], [0.0, -1.0]]), numpy.array([[1.0], [5.0], [0.0]])
    A1, b1 = numpy.array([[1.0, 0.0], [0.0, 0.0], [1.0, 1.0]]), numpy.array([[0.0], [7.0], [0.0]])
    none = (numpy.zeros((0, 2)), numpy.zeros((0, 1)))
    return Solution(None, [CriticalRegion(A0, b0, *none, sq[:, 1:] * 2.0, sq[:, :1] * 2.0, []), CriticalRegion(A1, b1, *none, bx[:, 1:] * 0.5, bx[:, :1] * 0.5, [])])


def test_output_range_direction_order_and_constant_rows(calls):
    sol = _solution()
    r = sol.output_range()
    off, ef, doff, d = calls[0]
    assert off.tolist() == [0, 4, 8] and numpy.allclose(ef, numpy.vstack([box_rows([0, 0], [1, 1]), box_rows([1, 0], [3, 1])]))
    assert doff.tolist() == [0, 6, 12]
    assert d.tolist() == [[2, -1], [-2, 1], [0, 0], [0, 0], [0, -1], [0, 1], [1, 0], [-1, 0], [0, 0], [0, 0], [1, 1], [-1, -1]]
    assert numpy.allclose(r.lo, [[0.0, 5.0, -1.0], [1.0, 7.0, 1.0]], atol=1e-12) and numpy.allclose(r.hi, [[3.0, 5.0, 0.0], [3.0, 7.0, 4.0]], atol=1e-12)
    assert r.lo[:, 1].tobytes() == r.hi[:, 1].tobytes() == numpy.array([5.0, 7.0]).tobytes() and r.stats['zero'] == 4 and r.stats['lps'] == 2 + 8
    assert not r.flag.any() and not r.thin.any() and numpy.allclose(r.arg_hi[0, 0], [1.0, 0.0]) and numpy.allclose(r.arg_lo[1, 2], [1.0, 0.0])
    lo, hi, region, theta = r.overall()
    assert numpy.allclose(lo, [0.0, 5.0, -1.0]) and numpy.allclose(hi, [3.0, 7.0, 4.0]) and region.tolist() == [[0, 0], [0, 1], [0, 1]]
    assert numpy.allclose(theta[2], [[0.0, 1.0], [3.0, 1.0]]) or numpy.allclose(theta[2][1], [3.0, 1.0])
    one = sol.output_range(outputs=[2])
    assert one.outputs == [2] and calls[-1][2].tolist() == [0, 2, 4] and numpy.allclose(one.hi[:, 0], [0.0, 4.0])


# ---- every ValueError is raised before _lib is touched ------------------------------------------------------------------------------------
def test_refusals_before_the_library(monkeypatch):
    def never(*a, **kw):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'support_rows', never)
    monkeypatch.setattr(_lib, 'reduce_rows', never)
    sq = box_rows([0, 0], [1, 1])
    off, d1 = numpy.array([0, 4]), numpy.array([[1.0, 0.0]])
    good = dict(row_off=off, rows=sq, n=2, dir_off=[0, 1], dirs=d1)
    nan_row = sq.copy()
    nan_row[1, 1] = numpy.nan
    for change, text in (({'n': 0}, 'outside 1..16'), ({'n': 17}, 'outside 1..16'), ({'tol': -1.0}, 'tol must be finite'), ({'tol': numpy.nan}, 'tol must be finite'),
                         ({'rows': nan_row}, 'rows must be finite'), ({'rows': sq * 2.0}, 'unit normals'), ({'row_off': [0, 0, 4], 'dir_off': [0, 0, 1]}, '1..512 rows'),
                         ({'row_off': [0, 516], 'rows': numpy.tile(sq, (129, 1))}, '1..512 rows'), ({'row_off': [1, 4]}, 'row_off'),
                         ({'dir_off': [1, 1]}, 'dir_off'), ({'dir_off': [0, 2]}, 'dir_off'), ({'dir_off': [0, 1, 1]}, 'dir_off'),
                         ({'row_off': [0, 2, 4], 'dir_off': [0, 2, 1], 'dirs': numpy.vstack([d1, d1])}, 'dir_off'),
                         ({'dirs': numpy.array([[numpy.nan, 0.0]])}, 'directions must be finite'), ({'dirs': numpy.array([[numpy.inf, 0.0]])}, 'directions must be finite'),
                         ({'dirs': numpy.ones((1, 3))}, 'dirs must be'), ({'start': numpy.array([[numpy.inf, 0.0]])}, 'start must be a finite'),
                         ({'start': numpy.zeros((2, 2))}, 'start must be a finite')):
        with pytest.raises(ValueError, match='support_of.*' + text):
            support_of(**dict(good, **change))
    P, zero = _poly(sq), Polytope(numpy.array([[1.0, 0.0], [0.0, 0.0]]), numpy.ones((2, 1)))
    with pytest.raises(ValueError, match='support: a polytope has no rows, or a row without a normal'):
        support(zero, d1)
    for wrong in ([1.0, 2.0, 3.0], numpy.ones((2, 3)), numpy.ones((1, 2, 2)), []):
        with pytest.raises(ValueError, match='Polytope.support: directions must be one direction'):
            P.support(wrong)
    for d in ([[1e-200, 0.0]], [[1e200, 1e200]], [[5e-324, 0.0]]):        # any finite direction is accepted
        with pytest.raises(AssertionError, match='the library was reached'):
            support(P, numpy.array(d))
    with pytest.raises(ValueError, match='support: no polytopes'):
        support([], d1)
    with pytest.raises(ValueError, match='support: 1 direction lists for 2 polytopes'):
        support([P, P], [d1])
    with pytest.raises(ValueError, match='different dimensions'):
        support([P, _poly(numpy.array([[1.0, 1.0], [1.0, -1.0]]))], d1)
    with pytest.raises(ValueError, match=r'pontryagin_difference: 1 polytopes Q for 2 polytopes P'):
        pontryagin_difference([P, P], [P])
    with pytest.raises(ValueError, match=r'pontryagin_difference: Q has 1 coordinates, P has 2'):
        pontryagin_difference(P, _poly(numpy.array([[1.0, 1.0], [1.0, -1.0]])))
    with pytest.raises(ValueError, match=r'pontryagin_difference: E must be a finite \[2, 2\] matrix'):
        pontryagin_difference(P, P, E=numpy.ones((2, 1)))
    with pytest.raises(ValueError, match='a row without a normal'):
        pontryagin_difference(P, zero)
    with pytest.raises(ValueError, match='containment: 2 inner and 1 outer polytopes: name the pairs'):
        containment([P, P], [P])
    with pytest.raises(ValueError, match='containment: a pair names a polytope out of range'):
        containment([P], [P], pairs=[(0, 1)])
    with pytest.raises(ValueError, match='containment: pairs must be'):
        containment([P], [P], pairs=[])
    with pytest.raises(ValueError, match='containment: the inner polytopes have 2 coordinates, the outer ones 1'):
        containment(P, _poly(numpy.array([[1.0, 1.0], [1.0, -1.0]])))
    sol = _solution()
    with pytest.raises(ValueError, match='output_range: tol must be finite'):
        sol.output_range(tol=-1.0)
    with pytest.raises(ValueError, match='output_range: outputs must be row indices of x in 0..2, got 3'):
        sol.output_range(outputs=[3])
    with pytest.raises(ValueError, match='output_range: the solution has no regions'):
        Solution(None, []).output_range()
    r = sol.critical_regions[0]
    many = Solution(None, [CriticalRegion(r.A, r.b, r.C, r.d, numpy.tile(r.E, (129, 1)), numpy.tile(r.f, (129, 1)), [])])
    with pytest.raises(ValueError, match='output_range: region 0 has more than 512 rows'):
        many.output_range()
    wide = Solution(None, [CriticalRegion(numpy.ones((1, 17)), numpy.ones((1, 1)), numpy.zeros((0, 17)), numpy.zeros((0, 1)), numpy.eye(17), numpy.ones((17, 1)), [])])
    with pytest.raises(ValueError, match='output_range: n_theta = 17 > 16'):
        wide.output_range()


def test_erosion_reference_stays_off_the_knife():
    """the seeds of the device test of pontryagin_difference with reduce_rows: the reference's erosion followed by the reference's
    reduction has no knife polytope beyond the share the reduction tests allow"""
    for case in sc.ERODE_SETS:
        polys, E, Q = sc.erosion_inputs(case)
        eroded = [ref.erosion(p, Q, E) for p in polys]
        assert not any(e[0] for e in eroded)
        want = rr.reduce_reference([e[1] for e in eroded], rc.TOL)
        assert sum(w.knife for w in want) <= 0.02 * len(polys) and not any(w.thin for w in want) and not any(w.wide for w in want)
