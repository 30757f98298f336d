"""Projections of polytopes on the device: the hand cases of tests/project_cases.py; seeded sets against the independent
CPU reference at tol = 1e-6, up to n = 16 and past 256 raw rows; without the reference: support values in 200 directions and along every
result row, membership of projected sample points, idempotence, determinism, start points, projecting in two calls; Minkowski sums, the
one-step controllable set of the double integrator, the library's refusals."""
import time

import numpy
import pytest
from scipy.optimize import linprog

import exit_cases as ec
import project_cases as pc
import project_reference as pr
import reduce_cases as rc
from ppopt_amd import _lib
from ppopt_amd.geometry import Polytope, controllable_pre, minkowski_sum, project_polytopes, project_rows_of, reduce_rows_of
from ppopt_amd.geometry import project as pj

pytestmark = pytest.mark.gpu

TOL = pc.TOL
KNIFE_SHARE = 0.02       # of a case's polytopes
HAND = pc.hand_cases()


def _support(rows, d):
    """max d.x over the rows [o | n] by scipy's HiGHS"""
    res = linprog(-numpy.asarray(d, dtype=float), A_ub=rows[:, 1:], b_ub=rows[:, 0], bounds=[(None, None)] * (rows.shape[1] - 1), method='highs')
    assert res.status == 0, res.message
    return -float(res.fun)


# ---- 1. the hand cases -----------------------------------------------------------------------------------------------------------------
def test_hand_cases():
    for n in (2, 3):
        cases = [c for c in HAND if c[1].shape[1] == n + 1]
        off, ef = ec.csr([c[1] for c in cases])
        r = project_rows_of(off, ef, n, list(range(n - 1)), tol=TOL)
        assert r.status.tolist() == [c[3] for c in cases], [c[0] for c in cases]
        assert r.peak.tolist() == [c[5] for c in cases]
        assert numpy.diff(r.row_off).tolist() == [0 if c[4] is None else len(c[4]) for c in cases]
        for q, c in enumerate(cases):
            want = pr.project_one(c[1], 1, TOL)
            assert r.wide[q] <= want.wide, c[0]
            if c[4] is not None:
                assert numpy.max(numpy.abs(r.rows_of(q) - c[4])) <= 1e-12, c[0]
                assert numpy.max(numpy.abs(numpy.linalg.norm(r.rows_of(q)[:, 1:], axis=1) - 1.0)) <= 1e-12
        s = r.stats
        assert s['polytopes'] == len(cases) and s['thin'] == sum(c[3] == pc.THIN for c in cases) and s['whole'] == sum(c[3] == pc.WHOLE for c in cases)
        assert s['too_large'] == sum(c[3] == pc.TOO_LARGE for c in cases)
    tri = [c for c in HAND if c[0] == 'triangle_x'][0][1]
    onto_y = Polytope(tri[:, 1:] * 2.0, tri[:, :1] * 2.0).project([1], tol=TOL)
    assert numpy.max(numpy.abs(onto_y.rows() - numpy.array([[0.0, -1.0], [1.0, 1.0]]))) <= 1e-12


def test_without_elimination_it_is_one_pass_of_reduce_rows():
    for n in (2, 1):
        cases = [c for c in rc.hand_cases() if c[1].shape[1] == n + 1]
        off, ef = ec.csr([c[1] for c in cases])
        r = project_rows_of(off, ef, n, list(range(n)), tol=TOL)
        red = reduce_rows_of(off, ef, n, tol=TOL)
        want = numpy.concatenate([numpy.asarray(c[2], dtype=bool) if not c[3] else numpy.zeros(len(c[1]), dtype=bool) for c in cases])
        assert r.rows.tobytes() == ef[want].tobytes()                      # the kept rows, bit for bit
        assert r.status.tolist() == [pj.THIN if c[3] else pj.OK for c in cases] == red.status.tolist()
        assert r.wide.tolist() == red.wide.tolist() and r.stats['lps'] == red.stats['lps'] and r.stats['pivots'] == red.stats['pivots']
        assert r.stats['steps'] == 0 and r.peak.tolist() == [0] * len(cases)


# ---- 2. seeded sets against the reference ------------------------------------------------------------------------------------------------
_CACHE = {}


def _set(case):
    """the polytopes, the reference's answer and the device run: computed once, shared, never modified"""
    if case not in _CACHE:
        n, n_elim = case[0], case[1]
        polys = pc.seeded_set(*case)
        t0 = time.perf_counter()
        want = pr.project_reference(polys, n_elim, TOL)
        ref_s = time.perf_counter() - t0
        off, ef = ec.csr(polys)
        got = project_rows_of(off, ef, n, list(range(n - n_elim)), tol=TOL)
        _CACHE[case] = (polys, want, got, off, ef, ref_s)
    return _CACHE[case]


def _against_the_reference(case):
    """Statuses and peaks equal; the kept rows in the same order within 1e-9 (1 + |o|): a row is a sum of products of rows scaled by a
    norm of at least nu >= 1e-4, a few ulp (1e-16) over nu per step and at most three steps: 1e-11, two decades below the bound."""
    polys, want, got, off, ef, ref_s = _set(case)
    knife = [q for q, w in enumerate(want) if w.knife]
    s = got.stats
    print(f'{case}: {len(polys)} polytopes, {len(ef)} rows, peak {int(got.peak.max())} -> {s["rows_after"]}, {len(knife)} knife polytopes, nu '
          f'{min(w.nu for w in want):.2e}, reference {ref_s:.2f} s; device: {s["steps"]} steps, {s["lps"]} LPs, {s["pivots"] / max(1, s["lps"]):.2f} pivots '
          f'per LP, {s["device_ms"]:.3f} ms ({1e6 * s["device_ms"] / max(1, s["lps"]):.0f} ns per LP), wall {s["wall_ms"]:.1f} ms')
    assert len(knife) <= KNIFE_SHARE * len(polys) and min(w.nu for w in want) >= 1e-4
    worst = 0.0
    for q, w in enumerate(want):
        if q in knife:
            continue
        assert got.status[q] == w.status and got.peak[q] == w.peak, (case, q)
        assert got.wide[q] <= w.wide, (case, q)
        rows = got.rows_of(q)
        assert rows.shape == w.rows.shape, (case, q, rows.shape, w.rows.shape)
        err = numpy.abs(rows - w.rows) / (1.0 + numpy.abs(w.rows[:, :1]))
        worst = max(worst, float(err.max()))
    print(f'  largest row difference {worst:.2e} (bound 1e-9)')
    assert worst <= 1e-9
    if not knife:
        assert s['polytopes'] == len(polys) and s['steps'] == case[1] * len(polys)
        assert s['lps'] == sum(len(w.lp) for w in want)
        if case[1] == 1:
            assert s['rows_made'] == sum(w.peak for w in want)


@pytest.mark.parametrize('case', pc.SETS, ids=pc.IDS)
def test_seeded_sets_against_the_reference(case):
    _against_the_reference(case)


def test_sixteen_coordinates_against_the_reference():
    _against_the_reference(pc.WIDE_DIM)


def test_more_than_256_raw_rows_against_the_reference():
    _against_the_reference(pc.MANY_ROWS)
    assert int(_set(pc.MANY_ROWS)[2].peak.max()) > 256


# ---- 3. without the reference --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [pc.SETS[1], pc.SETS[3]], ids=[pc.IDS[1], pc.IDS[3]])
def test_support_values_equal_those_of_the_polytope(case):
    """for 200 random unit directions of the kept space, shared among the polytopes, and for every result row: the support value of the
    result equals that of P in the lifted direction within 1e-8 (1 + |h|)"""
    polys, _, got, _, _, _ = _set(case)
    n, k = case[0], case[0] - case[1]
    rng = numpy.random.default_rng(7)
    D = rng.normal(size=(200, k))
    D /= numpy.linalg.norm(D, axis=1, keepdims=True)
    per = -(-200 // len(polys))
    worst = 0.0
    for q, P in enumerate(polys):
        res = got.rows_of(q)
        for d in list(D[q * per:(q + 1) * per]) + list(res[:, 1:]):
            h = _support(P, numpy.concatenate([d, numpy.zeros(n - k)]))
            worst = max(worst, abs(_support(res, d) - h) / (1.0 + abs(h)))
        for row in res:                                           # every result row is tight: its own right-hand side is the support value
            assert abs(_support(P, numpy.concatenate([row[1:], numpy.zeros(n - k)])) - row[0]) <= 1e-8 * (1.0 + abs(row[0]))
    print(f'{case}: largest support difference {worst:.2e} (bound 1e-8)')
    assert worst <= 1e-8


@pytest.mark.parametrize('case', [pc.SETS[1], pc.SETS[3]], ids=[pc.IDS[1], pc.IDS[3]])
def test_projected_points_lie_in_the_result(case):
    """20,000 uniform points of the polytopes of a set (rejection from the box c +- 2 they lie in), projected"""
    polys, _, got, _, _, _ = _set(case)
    n, k = case[0], case[0] - case[1]
    rng = numpy.random.default_rng(8)
    quota, total = -(-20000 // len(polys)), 0
    for q, P in enumerate(polys):
        axis = numpy.array([[P[(P[:, 1 + t] == s), 0][0] * s for s in (-1.0, 1.0)] for t in range(n)])     # the box rows: lower, upper
        pts = numpy.zeros((0, n))
        for _ in range(40):
            x = rng.uniform(axis[:, 0], axis[:, 1], size=(100000, n))
            pts = numpy.vstack([pts, x[numpy.all(x @ P[:, 1:].T <= P[:, 0], axis=1)]])
            if len(pts) >= quota:
                break
        pts = pts[:quota]
        assert len(pts) == quota
        res = got.rows_of(q)
        assert numpy.max(pts[:, :k] @ res[:, 1:].T - res[:, 0]) <= 1e-9
        total += len(pts)
    assert total >= 20000


def test_idempotent_deterministic_and_the_start_point():
    case = pc.SETS[3]
    polys, _, got, off, ef, _ = _set(case)
    n, k = case[0], case[0] - case[1]
    # projecting a result again onto all its coordinates removes nothing
    again = project_rows_of(got.row_off, got.rows, k, list(range(k)), tol=TOL)
    assert again.rows.tobytes() == got.rows.tobytes() and again.row_off.tolist() == got.row_off.tolist()
    # two runs are bit-identical
    twice = project_rows_of(off, ef, n, list(range(k)), tol=TOL)
    for name in ('rows', 'row_off', 'status', 'wide', 'peak', 'point'):
        assert getattr(twice, name).tobytes() == getattr(got, name).tobytes(), name
    assert {key: v for key, v in twice.stats.items() if not key.endswith('_ms')} == {key: v for key, v in got.stats.items() if not key.endswith('_ms')}
    # the interior point is interior to the result; a start point gives the same rows
    for q in range(len(polys)):
        assert numpy.min(got.rows_of(q)[:, 0] - got.rows_of(q)[:, 1:] @ got.point[q]) > TOL
    rng = numpy.random.default_rng(9)
    start = rng.uniform(-3.0, 3.0, size=(len(polys), n))
    other = project_rows_of(off, ef, n, list(range(k)), tol=TOL, start=start)
    assert other.row_off.tolist() == got.row_off.tolist() and other.status.tolist() == got.status.tolist()
    assert numpy.max(numpy.abs(other.rows - got.rows)) <= 1e-9


def test_two_calls_equal_one_call_as_a_set():
    case = pc.SETS[4]                                              # n = 5 onto 3 coordinates: first without 4, then without 3
    polys, _, got, off, ef, _ = _set(case)
    first = project_rows_of(off, ef, 5, [0, 1, 2, 3], tol=TOL)
    assert numpy.all(first.status == pj.OK)
    second = project_rows_of(first.row_off, first.rows, 4, [0, 1, 2], tol=TOL)
    assert second.status.tolist() == got.status.tolist()
    worst = 0.0
    for q in range(len(polys)):
        a, b = got.rows_of(q), second.rows_of(q)
        for mine, other in ((a, b), (b, a)):
            for row in mine:
                worst = max(worst, abs(_support(other, row[1:]) - row[0]) / (1.0 + abs(row[0])))
    print(f'two calls against one: largest support difference {worst:.2e} (bound 1e-8)')
    assert worst <= 1e-8


# ---- 4. the host layer on the device ----------------------------------------------------------------------------------------------------
def test_minkowski_sums_support_values_add():
    sq = ec.box_rows([0, 0], [1, 1])
    dm = numpy.array([[1.0, sx, sy] for sx in (1.0, -1.0) for sy in (1.0, -1.0)])
    octagon = minkowski_sum(Polytope(sq[:, 1:], sq[:, :1]), Polytope(dm[:, 1:], dm[:, :1]), tol=TOL)
    assert octagon.A.shape == (8, 2)
    for row in pc.octagon():
        s = numpy.linalg.norm(row[1:])
        assert abs(_support(octagon.rows(), row[1:] / s) - row[0] / s) <= 1e-8 * (1.0 + abs(row[0] / s))
    rng = numpy.random.default_rng(10)
    worst = 0.0
    for n, tangent, seed in ((2, 6, 70), (3, 6, 71)):
        a, b = pc.seeded_set(n, 0, tangent, 2, seed)
        both = minkowski_sum(Polytope(a[:, 1:], a[:, :1]), Polytope(b[:, 1:], b[:, :1]), tol=TOL)
        D = rng.normal(size=(40, n))
        D /= numpy.linalg.norm(D, axis=1, keepdims=True)
        for d in list(D) + list(both.A / numpy.linalg.norm(both.A, axis=1, keepdims=True)):
            h = _support(a, d) + _support(b, d)
            worst = max(worst, abs(_support(both.rows(), d) - h) / (1.0 + abs(h)))
    print(f'Minkowski sums: largest support difference {worst:.2e} (bound 1e-8)')
    assert worst <= 1e-8


def test_controllable_pre_of_the_double_integrator():
    """A = [[1, 1], [0, 1]], B = (0.5, 1), |u| <= 1, C = the box |x| <= 1.  A state is in Pre(C) iff the interval of the admissible u is
    not empty: |u| <= 1 and for either coordinate i -1 <= (A x)_i + B_i u <= 1, each a pair of bounds on the one input."""
    A, B = numpy.array([[1.0, 1.0], [0.0, 1.0]]), numpy.array([0.5, 1.0])
    box = ec.box_rows([-1, -1], [1, 1])
    U = Polytope(numpy.array([[1.0], [-1.0]]), numpy.array([[1.0], [1.0]]))
    got = controllable_pre(Polytope(box[:, 1:], box[:, :1]), A, B, U, tol=TOL)
    assert got.status.tolist() == [pj.OK]
    res = got.rows_of(0)
    x = numpy.random.default_rng(11).uniform(-4.0, 4.0, size=(20000, 2))
    Ax = x @ A.T
    lo = numpy.maximum(-1.0, numpy.max((-1.0 - Ax) / B, axis=1))
    hi = numpy.minimum(1.0, numpy.min((1.0 - Ax) / B, axis=1))
    slack = res[:, 0] - x @ res[:, 1:].T
    near = numpy.min(numpy.abs(slack), axis=1) <= 1e-6
    assert near.mean() <= 0.01
    inside = numpy.all(slack >= 0.0, axis=1)
    assert numpy.array_equal(inside[~near], (lo <= hi)[~near]) and 100 < inside.sum() < 19900
    # the integrator of the hand cases: x+ = x + u, |u| <= 1, C = [-1, 1]: [-2, 2]
    iv = Polytope(numpy.array([[1.0], [-1.0]]), numpy.array([[1.0], [1.0]]))
    one = controllable_pre(iv, [[1.0]], [1.0], iv, tol=TOL).rows_of(0)
    assert numpy.allclose(sorted(one.tolist()), [[2.0, -1.0], [2.0, 1.0]], atol=1e-12)


def test_the_librarys_refusals_surface_as_mpc_errors():
    sq = ec.box_rows([0, 0], [1, 1])
    off = numpy.array([0, 4], dtype=numpy.int64)
    call = lambda **kw: _lib.project_rows(kw.get('off', off), kw.get('ef', sq), kw.get('n_elim', 1), kw.get('start', None), kw.get('tol', TOL),
                                          kw.get('out_cap', 8))
    out_off, rows, status, wide, peak, point, stats = call()
    assert status.tolist() == [pj.OK] and out_off.tolist() == [0, 2] and rows.tolist() == [[1.0, 1.0], [0.0, -1.0]] and peak.tolist() == [3]
    assert stats['polytopes'] == 1 and stats['steps'] == 1 and stats['rows_made'] == 3
    small = call(out_cap=1)
    assert small[2].tolist() == [pj.TOO_LARGE] and len(small[1]) == 0               # more rows than out_cap: never a partial result
    long_row = sq.copy()
    long_row[0, 1] = 2.0
    for kw, text in ((dict(n_elim=2), 'n_elim must lie in 0..n - 1'), (dict(n_elim=-1), 'n_elim must lie'), (dict(tol=-1.0), 'tol must be finite'),
                     (dict(out_cap=0), 'out_cap must lie in 1..512'), (dict(out_cap=513), 'out_cap must lie'), (dict(ef=long_row), 'unit normals'),
                     (dict(off=numpy.array([0, 0, 4], dtype=numpy.int64)), r'1\.\.512 rows'), (dict(start=numpy.array([[numpy.inf, 0.0]])), 'start must be finite')):
        with pytest.raises(_lib.MpcError, match='mpc_project_rows.*' + text):
            call(**kw)
