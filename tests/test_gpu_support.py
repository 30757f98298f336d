"""Support functions on the device: the hand cases of tests/support_cases.py; seeded direction lists over the polytopes of
tests/reduce_cases.py against the independent CPU reference, up to n_theta = 16 and 512 rows; without the reference: feasibility of the
maximisers and the vertex maximum; independence of order, blocks and repetition; the bounding boxes of mpc_transition_boxes; and what is
built on it: Pontryagin differences, containment, Solution.output_range, robust_controllable_pre, the library's refusals."""
import ctypes
import time

import numpy
import pytest

import exit_cases as ec
import reduce_cases as rc
import reduce_reference as rr
import support_cases as sc
import support_reference as ref
from ppopt_amd import _lib
from ppopt_amd.geometry import (Polytope, containment, controllable_pre, pontryagin_difference, reduce_rows_of, robust_controllable_pre, support_of)
from ppopt_amd.geometry.polytope_operations import hit_and_run_batch
from ppopt_amd.geometry.vertices import vertices_of_rows

pytestmark = pytest.mark.gpu

TOL = 1e-8
BAND = 1e-6              # against the HiGHS reference (its own 1e-7 tolerances), as in test_gpu_reduce.py
KNIFE_SHARE = 0.02
# Measured on the device over every seeded set (printed by test_feasibility_and_vertex_maximum, recorded in DESIGN §3.28), times ten:
FEAS = 10 * 1.826e-14      # largest violation max_k (n_k.arg - o_k) / (1 + |o_k|); the finding limit is 1e-9
VERTEX = 10 * 4.097e-14    # largest |value - max_v d.v| / (1 + |value|); the finding limit is 1e-7
S_OK, S_EMPTY, S_THIN = 0, 1, 2      # ERODED_* of ppopt_amd/geometry/support.py


def _poly(rows):
    rows = numpy.asarray(rows, dtype=float)
    return Polytope(rows[:, 1:].copy(), rows[:, :1].copy())


# ---- 1. the hand cases -----------------------------------------------------------------------------------------------------------------
def test_hand_cases():
    for n_t, want_stats in ((2, dict(polytopes=6, thin=1, directions=27, zero=2, lps=6 + 10 + 4 + 3 + 5)), (1, dict(polytopes=1, thin=0, directions=3, zero=1, lps=3))):
        cases = [c for c in sc.hand_cases() if c[1].shape[1] == n_t + 1]
        off, ef = ec.csr([c[1] for c in cases])
        doff, d = ec.csr([c[2] for c in cases])
        r = support_of(off, ef, n_t, doff, d, tol=TOL)
        outside = support_of(off, ef, n_t, doff, d, tol=TOL, start=numpy.full((len(cases), n_t), 5.0))      # a start in none of them
        assert outside.dir_status.tobytes() == r.dir_status.tobytes() and outside.poly_status.tobytes() == r.poly_status.tobytes()
        for q, c in enumerate(cases):
            got, arg = r.values_of(q), r.args_of(q)
            for k, w in enumerate(c[3]):
                if w is not None and numpy.isfinite(w):
                    assert abs(outside.values_of(q)[k] - w) <= 1e-12, (c[0], k)
                    for a in (arg[k], outside.args_of(q)[k]):                  # a maximiser is a point of the polytope
                        assert numpy.all(c[1][:, 1:] @ a <= c[1][:, 0] + 1e-12), (c[0], k, a)
            if c[0] in ('away', 'cone'):
                # the default start is outside and the radius run ends unbounded before it reaches the polytope: flagged, and moved in
                assert r.wide[q] == 1 and numpy.all(c[1][:, 1:] @ r.point[q] <= c[1][:, 0] - 1.0)
            if c[0] != 'strip':
                assert numpy.all(c[1][:, 1:] @ outside.point[q] < c[1][:, 0]), c[0]
            assert r.dir_status[doff[q]:doff[q + 1]].tolist() == c[4], c[0]
            assert int(r.poly_status[q]) == (_lib.SUPPORT_THIN if c[0] == 'strip' else _lib.SUPPORT_OK)
            for k, (g, w) in enumerate(zip(got, c[3])):
                if w is None:
                    assert numpy.isnan(g) and numpy.all(numpy.isnan(arg[k])), c[0]
                elif numpy.isinf(w):
                    assert g == w, c[0]
                else:
                    assert abs(g - w) <= 1e-12 and abs(c[2][k] @ arg[k] - w) <= 1e-12, (c[0], k, g)
            if c[0] == 'square':
                assert got[-1] == 0.0 and arg[-1].tobytes() == r.point[q].tobytes()       # the zero direction: the interior point
            if c[0] != 'strip':
                assert numpy.all(c[1][:, 1:] @ r.point[q] < c[1][:, 0])
        assert {k: r.stats[k] for k in want_stats} == want_stats
        assert r.stats['wide'] == int(numpy.sum(r.dir_status == _lib.SUPPORT_UNBOUNDED)) + int(r.wide.sum())
    # directions of any finite length
    v, a = _poly(ec.box_rows([0, 0], [1, 1])).support([[1e-200, 0.0], [1e200, 1e200], [0.0, -5e-324], [-1e-200, 3e200]])
    assert numpy.allclose(v, [1e-200, 2e200, 0.0, 3e200], rtol=1e-12, atol=0)
    assert numpy.allclose(a[:, 0], [1, 1, a[2, 0], a[3, 0]], rtol=0, atol=1e-12) and numpy.allclose(a[:, 1], [a[0, 1], 1, 0, 1], rtol=0, atol=1e-12)
    assert numpy.all(a >= 0.0) and numpy.all(a <= 1.0 + 1e-12)          # the coordinate a direction does not weigh stays where it was
    # a disturbance set away from the origin moves the difference the other way
    e = _poly(ec.box_rows([0, 0], [1, 1])).erode(_poly(numpy.array([[-1.0, 1.0, 0.0], [3.0, -1.0, 0.0], [1.0, 0.0, 1.0], [1.0, 0.0, -1.0]])), reduce_rows=False)
    assert numpy.allclose(numpy.hstack([e.b, e.A]), ec.box_rows([3, 1], [2, 0]), rtol=0, atol=1e-12)
    v, a = _poly(ec.box_rows([0, 0], [1, 1]) * 3.0).support([[2.0, 2.0], [0.0, 0.0]])
    assert numpy.allclose(v, [4.0, 0.0], rtol=0, atol=1e-12) and numpy.allclose(a[0], [1.0, 1.0], rtol=0, atol=1e-12)


# ---- 2. seeded sets against the reference ------------------------------------------------------------------------------------------------
_CACHE = {}


def _set(case):
    """the polytopes, their direction lists, the reference's answers and the device run: computed once, shared, never modified"""
    if case not in _CACHE:
        polys, dirs = sc.seeded(case)
        t0 = time.perf_counter()
        want = [[ref.support(p, dk) for dk in d] for p, d in zip(polys, dirs)]
        thin = [(not u) and not r > TOL for u, r, _ in (ref.radius(p) for p in polys)]
        ref_s = time.perf_counter() - t0
        off, ef = ec.csr(polys)
        doff, d = ec.csr(dirs)
        got = support_of(off, ef, ef.shape[1] - 1, doff, d, tol=TOL)
        _CACHE[case] = (polys, dirs, want, thin, got, off, ef, doff, d, ref_s)
    return _CACHE[case]


@pytest.mark.parametrize('case', sc.CASES, ids=sc.IDS)
def test_seeded_sets_against_the_reference(case):
    """thin polytopes with these seeds (the reference alone, run on the CPU): none"""
    polys, dirs, want, thin, got, off, ef, doff, d, ref_s = _set(case)
    s = got.stats
    print(f'{case}: {len(polys)} polytopes, {len(ef)} rows, {len(d)} directions, reference {ref_s:.2f} s; device: {s["lps"]} LPs, '
          f'{s["pivots"] / max(1, s["lps"]):.2f} pivots per LP, {s["device_ms"]:.3f} ms ({1e6 * s["device_ms"] / max(1, s["lps"]):.0f} ns per LP)')
    assert not any(thin) and numpy.all(got.poly_status == _lib.SUPPORT_OK) and numpy.all(got.wide == 0)
    worst = 0.0
    for q in range(len(polys)):
        v, st = got.values_of(q), got.dir_status[doff[q]:doff[q + 1]]
        for k, (ws, wv, _) in enumerate(want[q]):
            assert int(st[k]) == (_lib.SUPPORT_UNBOUNDED if ws == ref.UNBOUNDED else _lib.SUPPORT_OK), (q, k)
            if ws == ref.UNBOUNDED:
                assert v[k] == numpy.inf
                continue
            nd = numpy.linalg.norm(dirs[q][k])
            worst = max(worst, abs(v[k] - wv) / (nd * (1.0 + abs(wv) / nd)))
            assert abs(v[k] - wv) <= BAND * nd * (1.0 + abs(wv) / nd), (q, k, v[k], wv)
    print(f'{case}: worst difference to the reference {worst:.3e} of the band unit')
    assert s['polytopes'] == len(polys) and s['thin'] == 0 and s['directions'] == len(d) and s['zero'] == 0 and s['lps'] == len(polys) + len(d)
    if case == 'rows512':
        assert polys[0].shape == (512, 17) and _lib.SUPPORT_MAX_ROWS == 512


# ---- 3. without the reference -------------------------------------------------------------------------------------------------------------
def test_feasibility_and_vertex_maximum():
    feas = vert = 0.0
    for case in sc.CASES:
        polys, dirs, want, thin, got, off, ef, doff, d, _ = _set(case)
        n = ef.shape[1] - 1
        for q, rows in enumerate(polys):
            a = got.args_of(q)
            feas = max(feas, float(numpy.max((a @ rows[:, 1:].T - rows[:, 0]) / (1.0 + numpy.abs(rows[:, 0])))))
        if case in sc.SINGLES or n > 5:
            continue
        vs = vertices_of_rows(off, ef, n)
        assert numpy.all(vs.status == 0)
        for q in range(len(polys)):
            ok = got.dir_status[doff[q]:doff[q + 1]] == _lib.SUPPORT_OK
            assert ok.all()                                                       # these sets are bounded
            top = numpy.max(dirs[q] @ vs.of(q).T, axis=1)
            vert = max(vert, float(numpy.max(numpy.abs(got.values_of(q) - top) / (1.0 + numpy.abs(top)))))
    print(f'largest feasibility violation {feas:.3e} (relative to 1 + |o|), largest difference to the vertex maximum {vert:.3e}')
    assert feas <= 1e-9 and vert <= 1e-7          # above these: a finding
    assert feas <= FEAS and vert <= VERTEX


# ---- 4. independence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [rc.SETS[1], rc.SETS[3]], ids=['n2', 'n5'])
def test_independence_of_order_blocks_and_repetition(case):
    polys, dirs, want, thin, got, off, ef, doff, d, _ = _set(case)
    q = 4                                                                          # the polytope with 200 directions: four blocks
    rows, dq, n = polys[q], dirs[q], ef.shape[1] - 1
    assert len(dq) == 200
    base = (got.values_of(q), got.args_of(q), got.dir_status[doff[q]:doff[q + 1]])
    cut = 77
    shapes = {'as is': ([rows], [dq], numpy.arange(200)), 'reversed': ([rows], [dq[::-1]], numpy.arange(200)[::-1]),
              'two copies': ([rows, rows], [dq[:cut], dq[cut:]], numpy.arange(200)), 'one each': ([rows] * 200, [dq[k:k + 1] for k in range(200)], numpy.arange(200))}
    for name, (ps, ds, order) in shapes.items():
        o2, e2 = ec.csr(ps)
        do2, d2 = ec.csr(ds)
        r = support_of(o2, e2, n, do2, d2, tol=TOL)
        assert r.value.tobytes() == base[0][order].tobytes(), name
        assert r.arg.tobytes() == numpy.ascontiguousarray(base[1][order]).tobytes(), name
        assert r.dir_status.tobytes() == numpy.ascontiguousarray(base[2][order]).tobytes(), name
        assert r.stats['lps'] == len(ps) + 200 and r.stats['polytopes'] == len(ps), name
    again = support_of(off, ef, n, doff, d, tol=TOL)
    for name in ('value', 'arg', 'dir_status', 'poly_status', 'wide', 'point'):
        assert getattr(again, name).tobytes() == getattr(got, name).tobytes(), name
    assert {k: again.stats[k] for k in ('lps', 'pivots', 'wide', 'zero')} == {k: got.stats[k] for k in ('lps', 'pivots', 'wide', 'zero')}
    moved = support_of(off, ef, n, doff, d, tol=TOL, start=got.point + 0.01)
    assert moved.dir_status.tobytes() == got.dir_status.tobytes() and moved.poly_status.tobytes() == got.poly_status.tobytes()


# ---- 5. the bounding boxes of an existing kernel --------------------------------------------------------------------------------------------
def _solved(name):
    import test_gpu_transition as tgt
    return tgt._case(name)


def _unit_rows(sol):
    ef, row_off, _ = sol._stacked()
    return row_off, ef / numpy.linalg.norm(ef[:, 1:], axis=1, keepdims=True)


def test_axis_directions_against_transition_boxes():
    sol, plant, _ = _solved('c2')
    off, ef = _unit_rows(sol)
    R, n = len(off) - 1, ef.shape[1] - 1
    axes = numpy.vstack([numpy.eye(n), -numpy.eye(n)])
    r = support_of(off, ef, n, numpy.arange(R + 1) * 2 * n, numpy.tile(axes, (R, 1)), tol=TOL)
    assert numpy.all(r.poly_status == _lib.SUPPORT_OK)
    box, flag, stats = _lib.transition_boxes(off, ef, numpy.tile(numpy.eye(n), (R, 1, 1)), numpy.zeros((R, n)), r.point)
    v = r.value.reshape(R, 2, n)
    upper, lower = v[:, 0], -v[:, 1]
    assert numpy.array_equal(numpy.isinf(upper), numpy.isinf(box[:, 1])) and numpy.array_equal(numpy.isinf(lower), numpy.isinf(box[:, 0]))
    for mine, theirs in ((upper, box[:, 1]), (lower, box[:, 0])):
        fin = numpy.isfinite(theirs)
        assert numpy.all(numpy.abs(mine[fin] - theirs[fin]) <= VERTEX * (1.0 + numpy.abs(theirs[fin])))
    print(f'c2: {R} regions; support {r.stats["lps"]} LPs, {r.stats["pivots"] / r.stats["lps"]:.2f} pivots per LP, {1e6 * r.stats["device_ms"] / r.stats["lps"]:.0f} ns per LP; '
          f'boxes {stats["lps"]} LPs, {stats["pivots"] / stats["lps"]:.2f} pivots per LP, {1e6 * stats["ms"] / stats["lps"]:.0f} ns per LP')


# ---- 6. Pontryagin differences --------------------------------------------------------------------------------------------------------------
def test_dyadic_boxes():
    P = [_poly(ec.box_rows([-1, -2], [3, 4]))]
    Q = _poly(ec.box_rows([-0.25, -0.5], [0.5, 0.125]))
    for reduce in (False, True):
        r = pontryagin_difference(P, Q, reduce_rows=reduce)
        assert r.status.tolist() == [0] and numpy.allclose(r.rows_of(0), ec.box_rows([-0.75, -1.5], [2.5, 3.875]), rtol=0, atol=1e-12)
    e = P[0].erode(Q)
    assert numpy.allclose(numpy.hstack([e.b, e.A]), ec.box_rows([-0.75, -1.5], [2.5, 3.875]), rtol=0, atol=1e-12)
    half = _poly(numpy.array([[1.0, 1.0, 0.0]]))
    r = pontryagin_difference(P, half)
    assert r.status.tolist() == [S_EMPTY] and len(r.rows) == 0
    with pytest.raises(ValueError, match='Polytope.erode: the difference is EMPTY'):
        P[0].erode(half)
    with pytest.raises(ValueError, match='Polytope.erode: the difference is THIN'):
        P[0].erode(_poly(ec.box_rows([-3, -3], [3, 3])))
    with pytest.raises(ValueError, match='Q is THIN'):
        P[0].erode(_poly(ec.box_rows([0, 0], [0, 1])))



@pytest.mark.parametrize('case', sc.ERODE_SETS, ids=sc.ERODE_IDS)
def test_seeded_erosion(case):
    polys, E, Qrows = sc.erosion_inputs(case)
    n = case[0]
    P, Q = [_poly(p) for p in polys], _poly(Qrows)
    raw = pontryagin_difference(P, Q, E=E, reduce_rows=False)
    off, ef = ec.csr(polys)
    unit = ef / numpy.linalg.norm(ef[:, 1:], axis=1, keepdims=True)
    assert numpy.all(raw.status == S_OK) and raw.row_off.tobytes() == off.tobytes()
    assert raw.rows[:, 1:].tobytes() == numpy.ascontiguousarray(unit[:, 1:]).tobytes()
    assert raw.rows[:, 0].tobytes() == (unit[:, 0] - raw.support).tobytes()
    # shared Q: the distinct directions were sent once; one Q per P gives the same bytes
    sent = numpy.unique(numpy.ascontiguousarray(unit[:, 1:] @ E), axis=0)
    assert raw.stats['directions'] == len(sent) < len(ef)
    per = pontryagin_difference(P, [Q] * len(P), E=E, reduce_rows=False)
    assert per.stats['directions'] == len(ef) and per.rows.tobytes() == raw.rows.tobytes() and per.status.tobytes() == raw.status.tobytes()
    # against the reference's values
    for q, p in enumerate(polys):
        empty, want = ref.erosion(p, Qrows, E)
        nd = numpy.linalg.norm(p[:, 1:] @ E, axis=1)
        assert not empty and numpy.all(numpy.abs(raw.rows_of(q)[:, 0] - want[:, 0]) <= BAND * nd * (1.0 + numpy.abs(p[:, 0] - want[:, 0]) / nd))
    # x + E q in P for sampled x of the result and every vertex q of Q
    qv = vertices_of_rows(numpy.array([0, len(Qrows)]), Qrows, 2).of(0)
    red = pontryagin_difference(P, Q, E=E, tol=rc.TOL, reduce_rows=True)
    centre = reduce_rows_of(raw.row_off, raw.rows, n, tol=rc.TOL).point
    rng = numpy.random.default_rng(50 + n)
    worst, inside = 0.0, 0
    for q, p in enumerate(polys):
        u = rng.normal(size=(400, n))
        x = centre[q] + u * (rng.uniform(0.0, 1.0, 400) / numpy.linalg.norm(u, axis=1))[:, None]
        for rows in (raw.rows_of(q), red.rows_of(q)):
            x = x[numpy.all(x @ rows[:, 1:].T <= rows[:, 0], axis=1)]
        inside += len(x)
        for v in qv:
            worst = max(worst, float(numpy.max(((x + E @ v) @ p[:, 1:].T - p[:, 0]) / (1.0 + numpy.abs(p[:, 0])))))
    print(f'n = {n}: {inside} sampled points of the differences, worst violation of x + E q in P {worst:.3e}')
    assert inside > 100 * len(polys) / 4 and worst <= FEAS
    # reduce_rows=True against the reference's erosion followed by the reference's reduction
    want = rr.reduce_reference([ref.erosion(p, Qrows, E)[1] for p in polys], rc.TOL)
    knife = [q for q, w in enumerate(want) if w.knife]
    assert len(knife) <= KNIFE_SHARE * len(polys) and numpy.all(red.status == S_OK)
    kept = reduce_rows_of(raw.row_off, raw.rows, n, tol=rc.TOL)
    assert red.rows.tobytes() == raw.rows[kept.kept].tobytes() and red.row_off.tobytes() == kept.row_off.tobytes()
    for q, w in enumerate(want):
        if q not in knife:
            assert kept.kept[off[q]:off[q + 1]].tolist() == w.kept.tolist(), q


# ---- 7. containment -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [rc.SETS[1], rc.SETS[3]], ids=['n2', 'n5'])
def test_containment_of_scaled_copies(case):
    polys, dirs, want, thin, got, off, ef, doff, d, _ = _set(case)
    polys = polys[:8]
    small = [sc.scaled_about(p, got.point[q], 0.9) for q, p in enumerate(polys)]
    large = [sc.scaled_about(p, got.point[q], 1.1) for q, p in enumerate(polys)]
    inner, outer = [_poly(p) for p in small + large + polys + polys], [_poly(p) for p in polys + polys + small + large]
    built = [True] * 8 + [False] * 8 + [False] * 8 + [True] * 8
    rows_in, rows_out = small + large + polys + polys, polys + polys + small + large
    c = containment(inner, outer, tol=TOL)

    def reference(i_rows, o_rows):
        """(excess, the band of test 2 for it: the largest band of a row's value)"""
        h = numpy.array([ref.support(i_rows, r[1:])[1] for r in o_rows])
        return float(numpy.max(h - o_rows[:, 0])), BAND * float(numpy.max(1.0 + numpy.abs(h)))
    refs = [reference(i, o) for i, o in zip(rows_in, rows_out)]
    assert all(abs(r[0] - TOL) > 1e-6 for r in refs)
    assert c.inside.tolist() == built == [r[0] <= TOL for r in refs]
    for k, r in enumerate(refs):
        assert abs(c.excess[k] - r[0]) <= r[1], k
    # pairs with repeats; an unbounded inner polytope
    pairs = [(0, 1), (8, 0), (0, 0), (0, 1), (8, 0)]
    p = containment(inner[:9], outer[:2], pairs=pairs, tol=TOL)
    prefs = [reference(rows_in[i], rows_out[j]) for i, j in pairs]
    assert all(abs(r[0] - TOL) > 1e-6 for r in prefs) and p.inside.tolist() == [r[0] <= TOL for r in prefs] and p.inside[2] and not p.inside[1]
    assert p.excess[0].tobytes() == p.excess[3].tobytes() and p.excess[1].tobytes() == p.excess[4].tobytes()
    assert p.excess[2].tobytes() == c.excess[0].tobytes() and p.witness[2].tobytes() == c.witness[0].tobytes() and p.row[2] == c.row[0]
    n = case[0]
    half = _poly(numpy.append(1.0, numpy.eye(n)[0])[None])
    u = containment(half, outer[0], tol=TOL)
    assert u.excess[0] == numpy.inf and not u.inside[0]
    assert outer[0].contains_polytope(inner[0]) and not inner[0].contains_polytope(outer[0])


# ---- 8. Solution.output_range and robust_controllable_pre ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['c2', 'c3_l4'])
def test_output_range_of_the_plants(name):
    sol, plant, _ = _solved(name)
    r = sol.output_range()
    R, K = r.lo.shape
    assert R == len(sol) and not r.thin.any() and not r.flag.any() and numpy.all(r.lo <= r.hi)
    _, _, laws = sol._stacked()
    b, A = laws[:, :, 0], laws[:, :, 1:]
    # the law at 2,000 hit-and-run points of the regions, located by the solution itself
    pts = hit_and_run_batch([Polytope(q.E, q.f) for q in sol.critical_regions], chains=-(-2000 // R), samples=1, n_steps=50, seed=31)[:, :, 0, :]
    th = numpy.ascontiguousarray(pts.transpose(1, 0, 2).reshape(-1, pts.shape[-1])[:2000])
    x, reg = sol.evaluate_batch(th)
    # the locator accepts a point within its tolerance of a region; the bounds hold for the points inside the region it names
    off, ef = _unit_rows(sol)
    found = reg >= 0
    for k in numpy.flatnonzero(found):
        rows = ef[off[reg[k]]:off[reg[k] + 1]]
        found[k] = numpy.all(rows[:, 1:] @ th[k] <= rows[:, 0])
    assert found.sum() > 1500
    slack = FEAS * (1.0 + numpy.abs(x[found]) + numpy.linalg.norm(A[reg[found]], axis=2) * (1.0 + numpy.linalg.norm(th[found], axis=1))[:, None])
    assert numpy.all(x[found] >= r.lo[reg[found]] - slack) and numpy.all(x[found] <= r.hi[reg[found]] + slack)
    # the extremes over the device's vertices
    vs = sol.vertices()
    listed = numpy.flatnonzero(vs.status == 0)
    assert len(listed) >= R // 2
    worst = 0.0
    for i in listed:
        val = vs.of(i) @ A[i].T + b[i]
        scale = 1.0 + numpy.abs(b[i]) + numpy.linalg.norm(A[i], axis=1) * (1.0 + numpy.linalg.norm(vs.of(i), axis=1).max())
        worst = max(worst, float(numpy.max(numpy.abs(val.max(axis=0) - r.hi[i]) / scale)), float(numpy.max(numpy.abs(val.min(axis=0) - r.lo[i]) / scale)))
    print(f'{name}: {R} regions, {K} rows, {r.stats["lps"]} LPs, {r.stats["zero"]} zero directions, worst difference to the vertex extremes {worst:.3e}')
    assert worst <= VERTEX
    const = ~numpy.any(A != 0.0, axis=2)
    assert r.stats['zero'] == 2 * int(const.sum()) and r.stats['lps'] == R + 2 * int((~const).sum())
    assert r.lo[const].tobytes() == r.hi[const].tobytes() == b[const].tobytes()
    lo, hi, region, theta = r.overall()
    assert lo.tobytes() == r.lo.min(axis=0).tobytes() and hi.tobytes() == r.hi.max(axis=0).tobytes()
    k = numpy.arange(K)
    assert numpy.all(r.lo[region[:, 0], k] == lo) and numpy.all(r.hi[region[:, 1], k] == hi)
    one = sol.output_range(outputs=[K - 1])
    assert one.lo[:, 0].tobytes() == r.lo[:, K - 1].tobytes() and one.hi[:, 0].tobytes() == r.hi[:, K - 1].tobytes()


def test_robust_controllable_pre_of_a_double_integrator():
    A, B = numpy.array([[1.0, 1.0], [0.0, 1.0]]), numpy.array([[0.5], [1.0]])
    U, W = _poly(numpy.array([[1.0, 1.0], [1.0, -1.0]])), _poly(ec.box_rows([-1e-3, -1e-3], [1e-3, 1e-3]))
    target, shrunk = _poly(ec.box_rows([-1, -1], [1, 1])), _poly(ec.box_rows([-1 + 1e-3, -1 + 1e-3], [1 - 1e-3, 1 - 1e-3]))
    robust = robust_controllable_pre(target, A, B, U, W)
    plain, inner = controllable_pre(target, A, B, U), controllable_pre(shrunk, A, B, U)
    assert robust.status.tolist() == plain.status.tolist() == inner.status.tolist() == [0]
    rp, pp, ip = robust.polytopes()[0], plain.polytopes()[0], inner.polytopes()[0]
    c = containment([rp, ip, pp], [pp, rp, rp], tol=1e-9)
    print(f'excess of robust in plain {c.excess[0]:.3e}, of pre(shrunk) in robust {c.excess[1]:.3e}, of plain in robust {c.excess[2]:.3e}')
    assert c.inside.tolist() == [True, True, False] and c.excess[0] < -1e-4
    gone = robust_controllable_pre([target, target], A, B, U, _poly(ec.box_rows([-2, -2], [2, 2])))
    assert gone.status.tolist() == [1, 1] and len(gone.rows) == 0


# ---- 9. the library's refusals ----------------------------------------------------------------------------------------------------------------
def test_library_refusals():
    """MPC_ERR_INVALID (MpcError with the library's message) before any launch; an empty batch is fine"""
    sq = ec.box_rows(numpy.zeros(2), numpy.ones(2))
    off, ef = ec.csr([sq, sq])
    doff, d = numpy.array([0, 2, 3]), numpy.array([[1.0, 0.0], [0.0, 0.0], [-1.0, 2.0]])
    call = lambda **kw: _lib.support_rows(kw.get('off', off), kw.get('ef', ef), kw.get('doff', doff), kw.get('d', d), kw.get('start', None), kw.get('tol', TOL))
    value, arg, ds, ps, wide, point, stats = call()
    assert value.tolist() == [1.0, 0.0, 2.0] and ds.tolist() == [0, 0, 0] and stats['polytopes'] == 2 and stats['lps'] == 4 and stats['zero'] == 1
    value, arg, ds, ps, wide, point, stats = call(doff=[0, 0, 0], d=numpy.zeros((0, 2)))          # no direction at all: statuses and points
    assert len(value) == 0 and ps.tolist() == [0, 0] and stats['polytopes'] == 2 and stats['lps'] == 2 and numpy.all(sq[:, 1:] @ point[0] < sq[:, 0])
    value, arg, ds, ps, wide, point, stats = call(off=[0], ef=numpy.zeros((0, 3)), doff=[0], d=numpy.zeros((0, 2)))
    assert len(value) == 0 and len(ps) == 0 and stats['polytopes'] == 0 and stats['ms'] == 0.0
    nan = ef.copy()
    nan[1, 1] = numpy.nan
    big = numpy.tile(sq, (129, 1))
    bad_d = lambda v: numpy.array([[1.0, 0.0], [0.0, 0.0], [v, 2.0]])
    for kw, text in (({'tol': -1.0}, 'tol must be finite'), ({'tol': numpy.nan}, 'tol must be finite'), ({'ef': nan}, 'finite with unit normals'),
                     ({'ef': ef * 2.0}, 'finite with unit normals'), ({'start': numpy.array([[numpy.inf, 0.0], [0.0, 0.0]])}, 'start must be finite'),
                     ({'off': [0, 0, 8]}, '1..512 rows'), ({'off': [0, 516], 'ef': big, 'doff': [0, 3]}, '1..512 rows'),
                     ({'d': bad_d(numpy.nan)}, 'dirs must be finite'), ({'d': bad_d(numpy.inf)}, 'dirs must be finite'),
                     ({'doff': [1, 2, 3]}, r'dir_off\[0\] must be 0'), ({'doff': [0, 4, 3]}, 'dir_off decreases'),
                     ({'off': [0, 2], 'ef': numpy.hstack([numpy.ones((2, 1)), numpy.eye(17)[:2]]), 'doff': [0, 0], 'd': numpy.zeros((0, 17))}, 'n_t must lie in 1..16')):
        with pytest.raises(_lib.MpcError, match='mpc_support_rows.*' + text):
            call(**kw)
    with pytest.raises(_lib.MpcError, match='row_off'):
        call(off=[1, 4, 8])
    # hole by hole through ctypes: every array the call needs
    L = _lib.load()
    o, e, do, dd = (numpy.ascontiguousarray(a) for a in (off, ef, numpy.asarray(doff, dtype=numpy.int64), d))
    val, st, pst, wd = numpy.zeros(3), numpy.zeros(3, dtype=numpy.int32), numpy.zeros(2, dtype=numpy.int32), numpy.zeros(2, dtype=numpy.int32)
    arrays = {'row_off': o, 'ef_rows': e, 'dir_off': do, 'dirs': dd, 'value': val, 'dir_status': st, 'poly_status': pst, 'wide': wd}

    def raw(missing=None, n_poly=2):
        p = {k: (None if k == missing else _lib._ptr(a)) for k, a in arrays.items()}
        return L.mpc_support_rows(0, 2, n_poly, p['row_off'], p['ef_rows'], p['dir_off'], p['dirs'], None, ctypes.c_double(TOL), p['value'], None,
                                  p['dir_status'], p['poly_status'], p['wide'], None, None, None)
    assert raw() == _lib.MPC_OK and val.tolist() == [1.0, 0.0, 2.0]
    for name in arrays:
        assert raw(missing=name) == _lib.MPC_ERR_INVALID and b'mpc_support_rows' in L.mpc_last_error(None), name
    assert L.mpc_support_rows(0, 2, 0, None, None, None, None, None, ctypes.c_double(TOL), None, None, None, None, None, None, None, None) == _lib.MPC_OK


# ---- the measurement (recorded in DESIGN §3.28, not gated) -----------------------------------------------------------------------------------
def test_measurement():
    def line(name, s, box):
        print(f'{name}: support {s["lps"]} LPs, {s["pivots"] / s["lps"]:.2f} pivots per LP, {s["device_ms"]:.3f} ms, {1e6 * s["device_ms"] / s["lps"]:.0f} ns per LP; '
              f'boxes {box["lps"]} LPs, {box["pivots"] / box["lps"]:.2f} pivots per LP, {box["ms"]:.3f} ms, {1e6 * box["ms"] / box["lps"]:.0f} ns per LP')

    def boxes(off, ef, point):
        R, n = len(off) - 1, ef.shape[1] - 1
        return _lib.transition_boxes(off, ef, numpy.tile(numpy.eye(n), (R, 1, 1)), numpy.zeros((R, n)), point)[2]
    for case in (rc.SETS[3], rc.SETS[4]):
        polys, dirs, want, thin, got, off, ef, doff, d, _ = _set(case)
        line(f'n{case[0]}', got.stats, boxes(off, ef, got.point))
    rows = rc.polytope(numpy.random.default_rng(5), 5, 9, 1, 0)
    assert len(rows) == 20
    g = numpy.random.default_rng(6).normal(size=(1_000_000, 5))
    off, ef = ec.csr([rows])
    r = support_of(off, ef, 5, numpy.array([0, len(g)]), g, tol=TOL, args=False)
    assert r.stats['lps'] == 1 + len(g) and numpy.all(r.dir_status == _lib.SUPPORT_OK) and r.arg is None
    line('one 20-row polytope, 10^6 directions', r.stats, boxes(off, ef, r.point))
