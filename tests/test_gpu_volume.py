"""Region volumes and centroids on the device (k_volume_walk) against closed forms, the numpy recursion of
tests/volume_reference.py and qhull: known and random polytopes up to 16 dimensions, cuts through vertices, affine maps, statuses, the
regions of solved programs, the exact coverage against a sampled one, the refusals and determinism.

Tolerances: volume relative 1e-10, centroid absolute 1e-10 (1 + |c|_inf), against either reference and the closed forms."""
import math
import warnings

import numpy
import pytest

import vertex_reference as vref
import volume_reference as ref
from ppopt_amd.geometry.polytope import Polytope
from ppopt_amd.geometry.vertices import EMPTY, NOT_POINTED, OK, OVERFLOW, UNBOUNDED, polytope_vertices
from ppopt_amd.geometry.volume import INCONSISTENT, TOO_LARGE, polytope_volumes, volumes_of_rows

pytestmark = pytest.mark.gpu

RTOL = 1e-10
LARGEST = {}            # group -> the largest relative volume difference seen (printed: pytest -s)


def _close(group, vol, want):
    d = abs(vol - want) / abs(want)
    LARGEST[group] = max(LARGEST.get(group, 0.0), d)
    print(f'{group}: volume {vol!r} against {want!r}: relative {d:.3e} (largest so far {LARGEST[group]:.3e})')
    return d <= RTOL


def _cen_close(c, want):
    c, want = numpy.asarray(c, dtype=float), numpy.asarray(want, dtype=float)
    return numpy.max(numpy.abs(c - want)) <= 1e-10 * (1 + numpy.max(numpy.abs(want)))


KNOWN = [('cube', n, vref.cube, lambda n: 2.0 ** n, lambda n: numpy.zeros(n)) for n in range(2, 9)] + \
        [('simplex', n, vref.simplex, lambda n: 1.0 / math.factorial(n), lambda n: numpy.full(n, 1.0 / (n + 1))) for n in range(2, 9)] + \
        [('cross', n, vref.cross_polytope, lambda n: 2.0 ** n / math.factorial(n), lambda n: numpy.zeros(n)) for n in range(3, 7)]


@pytest.mark.parametrize('name,n,make,volume,centre', KNOWN, ids=[f'{k[0]}{k[1]}' for k in KNOWN])
def test_known_polytopes(name, n, make, volume, centre):
    A, b, _ = make(n)
    rv = polytope_volumes(Polytope(A, b))
    assert rv.status.tolist() == [OK]
    assert _close('known', rv.volume[0], volume(n))
    assert _cen_close(rv.centroid[0], centre(n))
    # the count of the numpy recursion on the same vertices in the same order
    assert rv.simplices[0] == ref.reference(A, b, rv.vertices.of(0))[2]
    if name == 'simplex':
        assert rv.simplices[0] == 1
    assert rv.stats['simplices'] == rv.simplices[0] == rv.stats['max_simplices']


def _random(rng, n, cuts):
    """a scaled, shifted simplex cut by random rows through its interior (the generator of test_gpu_vertices)"""
    A, b, _ = vref.simplex(n)
    c = rng.normal(size=n)
    A = numpy.vstack([A, rng.normal(size=(cuts, n))])
    x0 = numpy.full(n, 1.0 / (n + 1))
    b = numpy.r_[b, A[n + 1:] @ x0 + rng.uniform(0.01, 0.2, size=cuts)]
    s = rng.uniform(0.5, 3.0)
    return A, s * b + A @ c        # {A (y - c) / s <= b} with y = s x + c


@pytest.mark.parametrize('n', [2, 3, 5, 8, 12, 16])
def test_random_polytopes(n):
    rng = numpy.random.default_rng(n)
    # 3 cuts at n = 12 and 16 give 4e5 and 2e6 simplices, minutes of the numpy recursion: one cut there (1e3 and 1e4 simplices, < 1 s)
    cuts = 1 if n > 8 else 6
    polys = [_random(rng, n, cuts) for _ in range(4)]
    A, b = polys[0]
    polys.append((numpy.vstack([A, 2 * A[:2], A[-1:]]), numpy.r_[b, 2 * b[:2] + 1.0, b[-1:]]))
    rv = polytope_volumes([Polytope(A, b) for A, b in polys])
    assert (rv.status == OK).all()
    for i, (A, b) in enumerate(polys[:4]):
        V = vref.brute_force(A, b) if n > 8 else vref.qhull(A, b)
        vol, cen, _ = ref.reference(A, b, V)
        assert _close(f'random n={n} (recursion)', rv.volume[i], vol), i
        assert _cen_close(rv.centroid[i], cen), i
        if n <= 8:
            assert _close(f'random n={n} (qhull)', rv.volume[i], ref.qhull_volume(V)), i
    assert rv.volume[4] == pytest.approx(rv.volume[0], rel=RTOL, abs=0) and _cen_close(rv.centroid[4], rv.centroid[0])


def test_cuts_through_vertices():
    polys, whole = [], []
    for make, n in ((vref.cube, 4), (vref.cross_polytope, 5)):
        A, b, _ = make(n)
        cut = numpy.zeros(n)
        cut[:2] = 1.0
        polys += [Polytope(numpy.vstack([A, cut]), numpy.r_[b, 0.0]), Polytope(numpy.vstack([A, -cut]), numpy.r_[b, 0.0])]
        whole.append(2.0 ** n if make is vref.cube else 2.0 ** n / math.factorial(n))
    for n in (3, 5):
        A, b, _ = vref.cube(n)
        cut = numpy.zeros(n)
        cut[0], cut[1] = 1.0, -1.0
        polys += [Polytope(numpy.vstack([A, cut]), numpy.r_[b, 0.0]), Polytope(numpy.vstack([A, -cut]), numpy.r_[b, 0.0])]
        whole.append(2.0 ** n)
    for k, w in enumerate(whole):                    # one batch per pair: a batch holds polytopes of one dimension
        rv = polytope_volumes(polys[2 * k:2 * k + 2])
        assert (rv.status == OK).all(), rv.status
        assert _close('cuts (sum)', rv.volume[0] + rv.volume[1], w)
        assert _close('cuts (half)', rv.volume[0], w / 2) and _close('cuts (half)', rv.volume[1], w / 2)


@pytest.mark.parametrize('n', [3, 6])
def test_affine_maps(n):
    rng = numpy.random.default_rng(100 + n)
    A, b = _random(rng, n, 6)
    Q1, Q2 = numpy.linalg.qr(rng.normal(size=(n, n)))[0], numpy.linalg.qr(rng.normal(size=(n, n)))[0]
    T = Q1 @ numpy.diag(rng.uniform(1.0, 9.0, size=n)) @ Q2
    assert numpy.linalg.cond(T) <= 10.0
    c = rng.normal(size=n)
    A2 = A @ numpy.linalg.inv(T)
    rv = polytope_volumes([Polytope(A, b), Polytope(A2, b + A2 @ c)])
    assert (rv.status == OK).all()
    assert _close('affine', rv.volume[1], abs(numpy.linalg.det(T)) * rv.volume[0])
    assert _cen_close(rv.centroid[1], T @ rv.centroid[0] + c)


def test_statuses():
    P2 = lambda A, b: Polytope(numpy.array(A, dtype=float), numpy.array(b, dtype=float))
    rv = polytope_volumes([P2([[1, 0], [0, 1]], [1, 1]),                              # a cone
                           P2([[1, 0], [-1, 0]], [1, 1]),                             # a slab
                           P2([[1, 0], [-1, 0], [0, 1], [0, -1]], [1, -2, 1, 1]),     # empty
                           P2([[1, 0], [-1, 0], [0, 1], [0, -1]], [0, 0, 1, 1]),      # a segment: no interior
                           P2([[1, 1], [-1, 0], [0, -1]], [1, 0, 0])])               # a triangle
    assert rv.status.tolist() == [UNBOUNDED, NOT_POINTED, EMPTY, EMPTY, OK]
    assert rv.volume[:4].tolist() == [numpy.inf, numpy.inf, 0.0, 0.0] and _close('statuses', rv.volume[4], 0.5)
    assert numpy.isnan(rv.centroid[:4]).all() and _cen_close(rv.centroid[4], [1 / 3, 1 / 3])
    assert rv.simplices.tolist() == [0, 0, 0, 0, 1]
    assert rv.stats['status_counts'] == [1, 1, 1, 2, 0, 0, 0]


def test_interval():
    rv = polytope_volumes(Polytope(numpy.array([[2.0], [-1.0]]), numpy.array([5.0, 0.5])))     # -0.5 <= x <= 2.5
    assert rv.status.tolist() == [OK] and rv.simplices.tolist() == [1]
    assert _close('interval', rv.volume[0], 3.0) and _cen_close(rv.centroid[0], [1.0])


def test_work_cap_and_overflow():
    A, b, _ = vref.cube(6)
    full = polytope_volumes(Polytope(A, b))
    assert full.status.tolist() == [OK] and full.simplices.tolist() == [720]
    capped = polytope_volumes(Polytope(A, b), max_simplices=100)
    assert capped.status.tolist() == [TOO_LARGE] and numpy.isnan(capped.volume[0]) and numpy.isnan(capped.centroid).all()
    assert capped.simplices.tolist() == [0] and capped.stats['status_counts'][TOO_LARGE] == 1
    exact = polytope_volumes(Polytope(A, b), max_simplices=720)
    assert exact.status.tolist() == [OK] and exact.volume[0] == full.volume[0]
    A, b, _ = vref.cube(8)
    over = polytope_volumes(Polytope(A, b), max_vertices=100, slab=18)
    assert over.status.tolist() == [OVERFLOW] and numpy.isnan(over.volume[0]) and numpy.isnan(over.centroid).all()


def test_row_sets_in_global_memory():
    """the product of two 60-gons: 120 rows and 3,600 vertices, (4 + 120) * 57 = 7,068 words of stack and row sets, over the 5,120 that
    fit the LDS of a wave, so the walk reads the row sets from the global slab; the volume is the product of the areas"""
    k = 60
    ang = 2 * numpy.pi * (numpy.arange(k) + 0.5) / k
    A = numpy.zeros((2 * k, 4))
    A[:k, 0], A[:k, 1] = numpy.cos(ang + 0.3), numpy.sin(ang + 0.3)             # each polygon: inradius 1, turned off the axes
    A[k:, 2], A[k:, 3] = numpy.cos(ang + 0.7), numpy.sin(ang + 0.7)
    rv = polytope_volumes(Polytope(A, numpy.ones(2 * k)))
    assert rv.status.tolist() == [OK] and len(rv.vertices.of(0)) == k * k
    assert (4 + 2 * k) * ((k * k + 63) // 64) > 5120
    assert _close('global row sets', rv.volume[0], (k * math.tan(numpy.pi / k)) ** 2)
    assert _cen_close(rv.centroid[0], numpy.zeros(4))


def test_value_errors():
    A, b, _ = vref.cube(3)
    with pytest.raises(ValueError, match='n_theta'):
        polytope_volumes(Polytope(*vref.cube(17)[:2]))
    with pytest.raises(ValueError, match='rows'):
        polytope_volumes(Polytope(numpy.vstack([A] * 43), numpy.r_[tuple([b] * 43)]))
    with pytest.raises(ValueError, match='finite'):
        polytope_volumes(Polytope(A, numpy.r_[b[:-1], numpy.inf]))
    with pytest.raises(ValueError, match='max_simplices'):
        polytope_volumes(Polytope(A, b), max_simplices=0)
    with pytest.raises(ValueError, match='budget'):
        polytope_volumes(Polytope(A, b), budget=64)
    with pytest.raises(ValueError, match='no polytopes'):
        polytope_volumes([])


def test_inconsistent_incidence_is_reported():
    """a vertex claimed by a facet it does not lie on: the face lattice breaks, and the answer is a status, not a number"""
    from ppopt_amd import _lib
    A, b, _ = vref.cube(3)
    P = Polytope(A, b)
    rv = polytope_vertices(P)
    inc = rv.incidence.copy()
    assert rv.of(0)[5].tolist() == [1.0, -1.0, 1.0]
    inc[5, 0] |= numpy.uint64(1 << 1)       # (1, -1, 1) also on x_1 <= 1: an edge of three vertices
    ef = P.rows()
    vol, cen, ns, st, _ = _lib.region_volumes([0, len(ef)], ef, 3, rv.offsets, rv.vertices, inc, rv.status)
    assert st.tolist() == [INCONSISTENT] and numpy.isnan(vol[0]) and numpy.isnan(cen).all() and ns.tolist() == [0]


_SOLVED = {}


def _solve(name):
    if name in _SOLVED:
        return _SOLVED[name]
    import bench
    from ppopt_amd import MPLP_Program, problem_generator as pg
    from ppopt_amd.mp_solvers import mpqp_hip_combi_graph, mpqp_hip_combinatorial
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if name == 'c1_mplp':
            d = pg.transport_mplp_data()
            prog = MPLP_Program(d['A'], d['b'], d['c'], d['H'], d['A_t'], d['b_t'], d['F'], equality_indices=list(d['equality_indices']))
            sol = solve_mpqp(prog, mpqp_algorithm.combinatorial)
        elif name == 'c2':
            sol = solve_mpqp(bench.build_program('c2'), mpqp_algorithm.combinatorial)
        elif name == 'c3_l4':
            sol = mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4)
        elif name == 'c3_graph':
            sol = mpqp_hip_combi_graph.solve_graph(bench.build_program('c3'))
        elif name == 'mi':
            from test_export import mixed_integer_solution
            sol = mixed_integer_solution('mpMIQP_market_problem')[0]
        elif name == 'c3_merged':
            sol = _solve('c3_l4').merge_regions(outputs=[0, 1])
        else:
            raise KeyError(name)
    _SOLVED[name] = sol
    return sol


@pytest.mark.parametrize('name', ['c2', 'c3_l4', 'c3_merged'])
def test_solved_regions(name):
    sol = _solve(name)
    vols = sol.volumes()
    assert len(vols) == len(sol.critical_regions) == len(vols.volume) == len(vols.centroid) == len(vols.simplices)
    good = numpy.flatnonzero(vols.status == OK)
    assert len(good) >= 0.99 * len(vols), vols.stats
    for i in good:
        assert _close(f'solved {name}', vols.volume[i], ref.qhull_volume(vols.vertices.of(i))), i      # qhull raises where it cannot: nothing is dropped
    ef, row_off, _ = sol._stacked()
    slack = ef[:, 0] - numpy.einsum('ij,ij->i', ef[:, 1:], numpy.repeat(vols.centroid, numpy.diff(row_off), axis=0))
    assert numpy.all(slack[numpy.repeat(vols.status == OK, numpy.diff(row_off))] > 0)


@pytest.mark.parametrize('name', ['c3_l4', 'c3_graph'])
def test_coverage(name):
    sol = _solve(name)
    cov = sol.coverage_volume()
    P = sol.program
    A_t, b_t = numpy.asarray(P.A_t, dtype=float), numpy.asarray(P.b_t, dtype=float).reshape(-1)
    box = polytope_vertices(Polytope(A_t, b_t)).of(0)
    pts = numpy.random.default_rng(0).uniform(box.min(axis=0), box.max(axis=0), size=(200_000, A_t.shape[1]))
    pts = pts[numpy.all(pts @ A_t.T <= b_t[None], axis=1)]
    p_hat = float(numpy.mean(sol.get_region_batch(pts) >= 0))
    band = 5 * math.sqrt(p_hat * (1 - p_hat) / len(pts)) + 1e-9
    print(f'{name}: fraction {cov.fraction!r}, sampled {p_hat!r} of {len(pts)} points, band {band:.3e}, {cov}')
    assert abs(cov.fraction - p_hat) <= band
    if name == 'c3_graph':
        assert cov.fraction <= 1 + 1e-9
    else:
        assert cov.fraction < 1


def test_refusals():
    lp, mi = _solve('c1_mplp'), _solve('mi')
    if lp.is_overlapping:
        with pytest.raises(ValueError, match='overlapping'):
            lp.coverage_volume()
    with pytest.raises(ValueError, match='mixed-integer'):
        mi.coverage_volume()
    for sol in (lp, mi):
        vols = sol.volumes()
        assert len(vols) == len(sol.critical_regions) and numpy.count_nonzero(vols.status == OK) > 0


def test_determinism():
    sol = _solve('c3_l4')
    ef, row_off, _ = sol._stacked()
    a = volumes_of_rows(row_off, ef, ef.shape[1] - 1)
    b = volumes_of_rows(row_off, ef, ef.shape[1] - 1)
    for k in ('volume', 'centroid', 'simplices', 'status'):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
