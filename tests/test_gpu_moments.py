"""Second moments of polytopes and regions on the device (k_volume_walk<NT, true>) against closed forms, the numpy
recursion and qhull's Delaunay triangulation of tests/moment_reference.py: known and random polytopes up to 16 dimensions, affine maps,
cuts through vertices, bit identity with the volume pass, the regions of solved programs, expected values against sampling, refusals.

Tolerances: volume relative 1e-10 and centroid absolute 1e-10 (1 + |c|_inf) as in test_gpu_volume; second moment
max |dM2| <= 1e-10 max |M2 reference|.  The largest difference of every group is printed (pytest -s) and kept in DESIGN §3.18."""
import math

import numpy
import pytest

import moment_reference as mref
import vertex_reference as vref
from ppopt_amd.geometry.moments import integrate_quadratic, moments_of_rows, polytope_moments
from ppopt_amd.geometry.polytope import Polytope
from ppopt_amd.geometry.vertices import EMPTY, NOT_POINTED, OK, UNBOUNDED
from ppopt_amd.geometry.volume import TOO_LARGE, polytope_volumes
from test_gpu_volume import _cen_close, _random, _solve

pytestmark = pytest.mark.gpu

RTOL = 1e-10
LARGEST = {}            # group -> the largest relative second-moment difference seen (printed: pytest -s)


def _m2_close(group, got, want):
    got, want = numpy.asarray(got, dtype=float), numpy.asarray(want, dtype=float)
    d = float(numpy.max(numpy.abs(got - want)) / numpy.max(numpy.abs(want)))
    LARGEST[group] = max(LARGEST.get(group, 0.0), d)
    print(f'{group}: second moment relative {d:.3e} (largest so far {LARGEST[group]:.3e})')
    return d <= RTOL and numpy.array_equal(got, numpy.swapaxes(got, -1, -2))


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.int64)


KNOWN = [('cube', n, vref.cube, mref.cube_m2) for n in range(2, 9)] + [('simplex', n, vref.simplex, mref.simplex_m2) for n in range(2, 9)] + \
        [('cross', n, vref.cross_polytope, mref.cross_m2) for n in range(3, 7)]


@pytest.mark.parametrize('name,n,make,m2', KNOWN, ids=[f'{k[0]}{k[1]}' for k in KNOWN])
def test_known_polytopes(name, n, make, m2):
    A, b, _ = make(n)
    mom = polytope_moments(Polytope(A, b))
    assert mom.status.tolist() == [OK]
    assert _m2_close('known', mom.second_moment[0], m2(n))


@pytest.mark.parametrize('n', [2, 3, 5, 8, 12, 16])
def test_random_polytopes(n):
    rng = numpy.random.default_rng(n)
    cuts = 1 if n > 8 else 6
    polys = [_random(rng, n, cuts) for _ in range(4)]
    A, b = polys[0]
    polys.append((numpy.vstack([A, 2 * A[:2], A[-1:]]), numpy.r_[b, 2 * b[:2] + 1.0, b[-1:]]))
    mom = polytope_moments([Polytope(A, b) for A, b in polys])
    assert (mom.status == OK).all()
    for i, (A, b) in enumerate(polys[:4]):
        V = vref.brute_force(A, b) if n > 8 else vref.qhull(A, b)
        m0, m1, m2 = mref.reference_moments(A, b, V)
        assert abs(mom.volume[i] - m0) <= RTOL * m0 and _cen_close(mom.centroid[i], m1 / m0), i
        assert _m2_close(f'random n={n} (recursion)', mom.second_moment[i], m2), i
        if n <= 5:
            assert _m2_close(f'random n={n} (delaunay)', mom.second_moment[i], mref.delaunay_moments(V)[2]), i
    assert _m2_close(f'random n={n} (duplicated rows)', mom.second_moment[4], mom.second_moment[0])


@pytest.mark.parametrize('n', [3, 6, 10])
def test_affine_maps(n):
    rng = numpy.random.default_rng(100 + n)
    A, b = _random(rng, n, 6 if n <= 8 else 1)
    Q1, Q2 = numpy.linalg.qr(rng.normal(size=(n, n)))[0], numpy.linalg.qr(rng.normal(size=(n, n)))[0]
    T = Q1 @ numpy.diag(rng.uniform(1.0, 9.0, size=n)) @ Q2
    t = rng.normal(size=n)
    A2 = A @ numpy.linalg.inv(T)
    mom = polytope_moments([Polytope(A, b), Polytope(A2, b + A2 @ t)])
    assert (mom.status == OK).all()
    M0, M1, M2 = mom.volume[0], mom.first_moment[0], mom.second_moment[0]
    want = abs(numpy.linalg.det(T)) * (T @ M2 @ T.T + numpy.outer(T @ M1, t) + numpy.outer(t, T @ M1) + M0 * numpy.outer(t, t))
    assert _m2_close('affine', mom.second_moment[1], want)


def test_additivity():
    for make, n, m2 in ((vref.cube, 4, mref.cube_m2), (vref.cross_polytope, 5, mref.cross_m2)):
        A, b, _ = make(n)
        cut = numpy.zeros(n)
        cut[:2] = 1.0
        mom = polytope_moments([Polytope(numpy.vstack([A, cut]), numpy.r_[b, 0.0]), Polytope(numpy.vstack([A, -cut]), numpy.r_[b, 0.0]), Polytope(A, b)])
        assert (mom.status == OK).all(), mom.status
        assert _m2_close('additivity', mom.second_moment[0] + mom.second_moment[1], mom.second_moment[2])
        assert _m2_close('additivity', mom.second_moment[0] + mom.second_moment[1], m2(n))


def _mixed_batch():
    P2 = lambda A, b: Polytope(numpy.array(A, dtype=float), numpy.array(b, dtype=float))
    A, b, _ = vref.cube(2)
    ang = 2 * numpy.pi * (numpy.arange(40) + 0.5) / 40
    return [P2([[1, 0], [0, 1]], [1, 1]),                              # a cone: UNBOUNDED
            P2([[1, 0], [-1, 0]], [1, 1]),                             # a slab: NOT_POINTED
            P2([[1, 0], [-1, 0], [0, 1], [0, -1]], [1, -2, 1, 1]),     # EMPTY
            P2([[1, 1], [-1, 0], [0, -1]], [1, 0, 0]),                 # a triangle
            Polytope(A, b + numpy.array([0.5, 0.0, 0.25, 0.0])),       # a shifted square
            P2(numpy.c_[numpy.cos(ang), numpy.sin(ang)], numpy.ones(40))]    # a 40-gon: 38 simplices


def test_bit_identity_with_the_volume_pass():
    polys = _mixed_batch()
    for cap, want in ((None, [UNBOUNDED, NOT_POINTED, EMPTY, OK, OK, OK]), (10, [UNBOUNDED, NOT_POINTED, EMPTY, OK, OK, TOO_LARGE])):
        vol, mom = polytope_volumes(polys, max_simplices=cap), polytope_moments(polys, max_simplices=cap)
        again = polytope_moments(polys, max_simplices=cap)
        assert mom.status.tolist() == want
        for k in ('volume', 'centroid'):
            assert numpy.array_equal(_bits(getattr(mom, k)), _bits(getattr(vol, k))), k
            assert numpy.array_equal(_bits(getattr(mom, k)), _bits(getattr(again, k))), k
        assert numpy.array_equal(mom.simplices, vol.simplices) and numpy.array_equal(mom.status, vol.status)
        assert numpy.array_equal(_bits(mom.second_moment), _bits(again.second_moment))
        assert numpy.isnan(mom.second_moment[:2]).all() and not mom.second_moment[2].any()
        assert _m2_close('statuses', mom.second_moment[3], mref.simplex_m2(2))
        assert numpy.isnan(mom.second_moment[5]).all() == (cap is not None)
        assert mom.stats['status_counts'] == vol.stats['status_counts'] and mom.stats['simplices'] == vol.stats['simplices']
    # several chunks (a budget of 1,700 bytes: the 40-gon takes 1,620 of them, the triangle and the square 320) give the bits of one chunk
    from ppopt_amd import _lib
    rv = mom.vertices
    off = numpy.concatenate([[0], numpy.cumsum([len(p.rows()) for p in polys])])
    ef = numpy.vstack([p.rows() for p in polys])
    whole = _lib.region_moments(off, ef, 2, rv.offsets, rv.vertices, rv.incidence, rv.status)
    chunks = _lib.region_moments(off, ef, 2, rv.offsets, rv.vertices, rv.incidence, rv.status, budget=1700)
    assert chunks[5]['launches'] > whole[5]['launches']
    for k in range(3):
        assert numpy.array_equal(_bits(chunks[k]), _bits(whole[k])), k
    assert numpy.array_equal(chunks[3], whole[3]) and numpy.array_equal(chunks[4], whole[4])


def test_interval():
    iv = Polytope(numpy.array([[2.0], [-1.0]]), numpy.array([5.0, 0.5]))     # -0.5 <= x <= 2.5
    mom, vol = polytope_moments(iv), polytope_volumes(iv)
    assert mom.status.tolist() == [OK] and mom.simplices.tolist() == [1]
    assert numpy.array_equal(_bits(mom.volume), _bits(vol.volume)) and numpy.array_equal(_bits(mom.centroid), _bits(vol.centroid))
    assert _m2_close('interval', mom.second_moment[0], [[(2.5 ** 3 + 0.5 ** 3) / 3]])


def test_row_sets_in_global_memory():
    """the product of two 60-gons of test_gpu_volume.test_row_sets_in_global_memory: its row sets do not fit the LDS of a wave, so the
    walk reads them from the global slab.  Volume and centroid are the bits of the volume pass; the second moment is the product
    form: blocks area_2 * M2(polygon_1) and area_1 * M2(polygon_2), computed on the device from the polygons, whose row sets are in LDS"""
    k = 60
    ang = 2 * numpy.pi * (numpy.arange(k) + 0.5) / k
    A = numpy.zeros((2 * k, 4))
    A[:k, 0], A[:k, 1] = numpy.cos(ang + 0.3), numpy.sin(ang + 0.3)
    A[k:, 2], A[k:, 3] = numpy.cos(ang + 0.7), numpy.sin(ang + 0.7)
    P = Polytope(A, numpy.ones(2 * k))
    mom, vol = polytope_moments(P), polytope_volumes(P)
    assert mom.status.tolist() == [OK] and (4 + 2 * k) * ((k * k + 63) // 64) > 5120
    assert numpy.array_equal(_bits(mom.volume), _bits(vol.volume)) and numpy.array_equal(_bits(mom.centroid), _bits(vol.centroid))
    assert numpy.array_equal(mom.simplices, vol.simplices)
    gons = polytope_moments([Polytope(A[:k, :2], numpy.ones(k)), Polytope(A[k:, 2:], numpy.ones(k))])
    assert (gons.status == OK).all()
    want = numpy.zeros((4, 4))
    want[:2, :2], want[2:, 2:] = gons.volume[1] * gons.second_moment[0], gons.volume[0] * gons.second_moment[1]
    assert _m2_close('global row sets', mom.second_moment[0], want)
    # the polygons themselves against the closed form of a regular k-gon of inradius 1: M2 = area (1 / 4) (1 + tan^2(pi / k) / 3) I
    tan = math.tan(numpy.pi / k)
    assert _m2_close('global row sets', gons.second_moment[0], k * tan * 0.25 * (1 + tan * tan / 3) * numpy.eye(2))


@pytest.mark.parametrize('name', ['c2', 'c3_l4'])
def test_solved_regions(name):
    sol = _solve(name)
    mom, vol = sol.moments(), sol.volumes()
    assert len(mom) == len(sol.critical_regions)
    for k in ('volume', 'centroid'):
        assert numpy.array_equal(_bits(getattr(mom, k)), _bits(getattr(vol, k))), k
    assert numpy.array_equal(mom.simplices, vol.simplices) and numpy.array_equal(mom.status, vol.status)
    good = numpy.flatnonzero(mom.status == OK)
    assert len(good) >= 0.99 * len(mom), mom.stats
    ef, row_off, _ = sol._stacked()
    ref = numpy.full(mom.second_moment.shape, numpy.nan)
    ref0, ref1 = numpy.full(len(mom), numpy.nan), numpy.full(mom.centroid.shape, numpy.nan)
    for i in good:
        rows = ef[row_off[i]:row_off[i + 1]]
        ref0[i], ref1[i], ref[i] = mref.reference_moments(rows[:, 1:], rows[:, 0], mom.vertices.of(i))
        assert _m2_close(f'solved {name}', mom.second_moment[i], ref[i]), i
    if sol.is_overlapping:
        # solve_mpqp flags every solution it returns as overlapping, as the reference does; the regions of a strictly convex mpQP do
        # not overlap, and expected_values refuses by the flag: the same program and regions without it
        from ppopt_amd import Solution
        assert numpy.linalg.eigvalsh(sol.program.Q).min() > 0
        sol = Solution(sol.program, sol.critical_regions, is_overlapping=False, point_location_tolerance=sol.point_location_tolerance)
    ev = sol.expected_values()
    Qv, qv, rv = sol.value_function()
    want = numpy.array([0.5 * numpy.sum(Qv[i] * ref[i]) + qv[i] @ ref1[i] + rv[i] * ref0[i] for i in good])
    got = ev.objective_integral_by_region[good]
    d = float(numpy.max(numpy.abs(got - want)) / numpy.max(numpy.abs(want)))
    print(f'solved {name}: objective integral by region relative {d:.3e}')
    assert d <= RTOL
    assert numpy.array_equal(got, integrate_quadratic(mom, Qv, qv, rv)[good])
    assert ev.ok == bool(numpy.isin(mom.status, (OK, EMPTY)).all()) and abs(ev.total - mom.volume[good].sum()) <= RTOL * ev.total
    assert abs(ev.objective_integral - want.sum()) <= RTOL * numpy.abs(want).sum()


@pytest.mark.parametrize('name', ['c3_l4', 'c3_graph'])
def test_expected_values_against_sampling(name):
    from ppopt_amd.geometry.vertices import polytope_vertices
    sol = _solve(name)
    ev = sol.expected_values()
    P = sol.program
    A_t, b_t = numpy.asarray(P.A_t, dtype=float), numpy.asarray(P.b_t, dtype=float).reshape(-1)
    box = polytope_vertices(Polytope(A_t, b_t)).of(0)
    pts = numpy.random.default_rng(0).uniform(box.min(axis=0), box.max(axis=0), size=(200_000, A_t.shape[1]))
    pts = pts[numpy.all(pts @ A_t.T <= b_t[None], axis=1)]
    x, region = sol.evaluate_batch(pts)
    keep = region >= 0
    x, th = x[keep], pts[keep]
    Q, H, c = numpy.asarray(P.Q, dtype=float), numpy.asarray(P.H, dtype=float), numpy.asarray(P.c, dtype=float).reshape(-1)
    J = 0.5 * numpy.einsum('pi,ij,pj->p', x, Q, x) + numpy.einsum('pt,xt,px->p', th, H, x) + x @ c + float(numpy.asarray(P.c_c).reshape(-1)[0]) \
        + th @ numpy.asarray(P.c_t, dtype=float).reshape(-1) + 0.5 * numpy.einsum('pi,ij,pj->p', th, numpy.asarray(P.Q_t, dtype=float), th)
    N = len(J)
    band = 5 * J.std(ddof=1) / math.sqrt(N) + 1e-9
    print(f'{name}: objective mean {ev.objective_mean!r}, sampled {J.mean()!r} of {N} points, band {band:.3e}; {ev.status_counts}')
    assert abs(ev.objective_mean - J.mean()) <= band
    xb = 5 * x.std(axis=0, ddof=1) / math.sqrt(N) + 1e-9
    print(f'{name}: x mean {ev.x_mean}, sampled {x.mean(axis=0)}, bands {xb}')
    assert numpy.all(numpy.abs(ev.x_mean - x.mean(axis=0)) <= xb)
    assert numpy.all(numpy.linalg.eigvalsh(ev.x_cov) >= -1e-9 * numpy.trace(ev.x_cov)) and numpy.all(numpy.linalg.eigvalsh(ev.theta_cov) > 0)


def test_refusals():
    lp, mi, merged, src = _solve('c1_mplp'), _solve('mi'), _solve('c3_merged'), _solve('c3_l4')
    assert lp.is_overlapping
    with pytest.raises(ValueError, match='overlapping'):
        lp.expected_values()
    with pytest.raises(ValueError, match='mixed-integer'):
        mi.expected_values()
    with pytest.raises(ValueError, match='merged'):
        merged.value_function()
    with pytest.raises(ValueError, match='merged'):
        merged.expected_values()
    a, b = merged.moments(), src.moments()
    ga, gb = a.status == OK, b.status == OK
    print(f'merged: {ga.sum()} of {len(ga)} regions OK, source: {gb.sum()} of {len(gb)}')
    assert _m2_close('merged total', a.second_moment[ga].sum(axis=0), b.second_moment[gb].sum(axis=0))


def test_value_errors():
    A, b, _ = vref.cube(3)
    with pytest.raises(ValueError, match='n_theta'):
        polytope_moments(Polytope(*vref.cube(17)[:2]))
    with pytest.raises(ValueError, match='rows'):
        polytope_moments(Polytope(numpy.vstack([A] * 43), numpy.r_[tuple([b] * 43)]))
    with pytest.raises(ValueError, match='finite'):
        polytope_moments(Polytope(A, numpy.r_[b[:-1], numpy.inf]))
    with pytest.raises(ValueError, match='max_simplices'):
        polytope_moments(Polytope(A, b), max_simplices=0)
    with pytest.raises(ValueError, match='budget'):
        polytope_moments(Polytope(A, b), budget=64)
    with pytest.raises(ValueError, match='no polytopes'):
        polytope_moments([])
    with pytest.raises(ValueError, match='max_simplices'):
        moments_of_rows([0, len(A)], numpy.c_[b, A], 3, max_simplices=-1)
