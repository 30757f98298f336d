"""Vertex enumeration on the device (k_region_vertices) against the independent references of tests/vertex_reference.py:
hand polytopes, random polytopes up to 16 dimensions, redundant and duplicate rows, the statuses of unbounded, slab, empty and
lower-dimensional inputs, the overflow repeat, the regions of solved programs (feasibility, incidence, rank, the reference's sets) and
determinism."""
import warnings

import numpy
import pytest

import vertex_reference as ref
from ppopt_amd.geometry.polytope import Polytope
from ppopt_amd.geometry.vertices import EMPTY, NOT_POINTED, OK, OVERFLOW, UNBOUNDED, polytope_vertices

pytestmark = pytest.mark.gpu

KNOWN = [('cube', n, ref.cube) for n in range(2, 9)] + [('simplex', n, ref.simplex) for n in range(2, 9)] + \
        [('cross', n, ref.cross_polytope) for n in range(3, 7)]


@pytest.mark.parametrize('name,n,make', KNOWN, ids=[f'{k}{n}' for k, n, _ in KNOWN])
def test_known_polytopes(name, n, make):
    A, b, V = make(n)
    rv = polytope_vertices(Polytope(A, b))
    assert rv.status.tolist() == [OK]
    assert ref.same_set(rv.of(0), V, tol=1e-9)
    assert len(rv.rays) == 0


def test_cyclic_polytope():
    A, b, V = ref.cyclic_polytope(4, 9)
    rv = polytope_vertices(Polytope(A, b))
    assert rv.status.tolist() == [OK] and ref.same_set(rv.of(0), V, tol=1e-7)


def _random(rng, n, cuts):
    """a scaled, shifted simplex cut by random rows through its interior"""
    A, b, _ = ref.simplex(n)
    c = rng.normal(size=n)
    A = numpy.vstack([A, rng.normal(size=(cuts, n))])
    x0 = numpy.full(n, 1.0 / (n + 1))
    b = numpy.r_[b, A[n + 1:] @ x0 + rng.uniform(0.01, 0.2, size=cuts)]
    s = rng.uniform(0.5, 3.0)
    return A, s * b + A @ c        # {A (y - c) / s <= b} with y = s x + c


@pytest.mark.parametrize('n', [2, 3, 5, 8, 12, 16])
def test_random_polytopes(n):
    rng = numpy.random.default_rng(n)
    cuts = 3 if n > 8 else 6
    polys = [_random(rng, n, cuts) for _ in range(4)]
    # redundant rows (a scaled copy loosened) and an exact duplicate row
    A, b = polys[0]
    polys.append((numpy.vstack([A, 2 * A[:2], A[-1:]]), numpy.r_[b, 2 * b[:2] + 1.0, b[-1:]]))
    rv = polytope_vertices([Polytope(A, b) for A, b in polys])
    assert (rv.status == OK).all()
    for i, (A, b) in enumerate(polys):
        want = ref.brute_force(A, b) if n > 8 else ref.qhull(A, b)
        assert ref.same_set(rv.of(i), want, tol=1e-7), (i, len(rv.of(i)), len(want))
    assert ref.same_set(rv.of(4), rv.of(0), tol=1e-12)


def test_statuses_and_rays():
    P2 = lambda A, b: Polytope(numpy.array(A, dtype=float), numpy.array(b, dtype=float))
    rv = polytope_vertices([P2([[1, 0], [0, 1]], [1, 1]),                              # a cone: vertex (1, 1), rays -e1, -e2
                            P2([[1, 0], [-1, 0]], [1, 1]),                             # a slab: no vertex
                            P2([[1, 0], [-1, 0], [0, 1], [0, -1]], [1, -2, 1, 1]),     # empty
                            P2([[1, 0], [-1, 0], [0, 1], [0, -1]], [0, 0, 1, 1]),      # a segment: no interior
                            P2([[1, 1], [-1, 0], [0, -1]], [1, 0, 0])])               # a triangle
    assert rv.status.tolist() == [UNBOUNDED, NOT_POINTED, EMPTY, EMPTY, OK]
    assert numpy.allclose(rv.of(0), [[1.0, 1.0]])
    assert ref.same_set(rv.rays_of(0), [[-1.0, 0.0], [0.0, -1.0]], tol=1e-12)
    assert ref.same_set(rv.of(4), [[0, 0], [1, 0], [0, 1]], tol=1e-12)
    assert numpy.diff(rv.offsets).tolist() == [1, 0, 0, 0, 3] and numpy.diff(rv.ray_offsets).tolist() == [2, 0, 0, 0, 0]


def test_overflow_repeat_and_budget():
    A, b, V = ref.cube(8)
    big = polytope_vertices(Polytope(A, b))
    small = polytope_vertices(Polytope(A, b), slab=18)
    assert small.stats['repeats'] >= 1 and small.status.tolist() == [OK]
    assert numpy.array_equal(small.vertices, big.vertices) and numpy.array_equal(small.incidence, big.incidence)
    capped = polytope_vertices(Polytope(A, b), slab=18, max_vertices=100)
    assert capped.status.tolist() == [OVERFLOW] and len(capped.vertices) == 0 and capped.stats['overflow'] == 1


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
        elif name == 'c4_l4':
            sol = mpqp_hip_combinatorial.solve(bench.build_program('c4'), max_levels=4)
        elif name == 'mi':
            from test_export import mixed_integer_solution
            sol = mixed_integer_solution('mpMIQP_market_problem')[0]
        elif name == 'c3_merged':
            sol = _solve('c3_l4').merge_regions(outputs=[0, 1])
        else:
            raise KeyError(name)
    _SOLVED[name] = sol
    return sol


@pytest.mark.parametrize('name', ['c1_mplp', 'c2', 'c3_l4', 'c3_graph', 'c4_l4', 'mi', 'c3_merged'])
def test_solved_regions(name):
    sol = _solve(name)
    rv = sol.vertices()
    ef, row_off, _ = sol._stacked()
    n_t = ef.shape[1] - 1
    assert len(rv) == len(sol.critical_regions)
    assert rv.stats['overflow'] == 0, rv.stats
    n_reg = len(rv)
    sample = range(n_reg) if n_reg <= 1000 or name != 'c4_l4' else numpy.random.default_rng(0).choice(n_reg, 40, replace=False)
    checked = 0
    for i in range(n_reg):
        f, E = ef[row_off[i]:row_off[i + 1], 0], ef[row_off[i]:row_off[i + 1], 1:]
        V = rv.of(i)
        if rv.status[i] != OK:
            continue
        slack = f[None] - V @ E.T
        assert numpy.all(slack >= -1e-7 * (1 + numpy.abs(f))[None]), (i, slack.min())
        thr = 1e-9 * (1 + numpy.abs(f))[None]
        tight = numpy.abs(slack) <= thr
        clear = numpy.abs(numpy.abs(slack) - thr) > 1e-12 * (1 + numpy.abs(f))[None]
        inc = rv.incidence_of(i)
        bits = ((inc[:, numpy.arange(len(f)) // 64] >> (numpy.arange(len(f)) % 64).astype(numpy.uint64)) & numpy.uint64(1)).astype(bool)
        assert numpy.array_equal(bits[clear], tight[clear]), i
        for k in range(len(V)):
            assert numpy.linalg.matrix_rank(E[bits[k]], tol=1e-8) == n_t, (i, k)
        if (n_reg <= 1000 and name != 'c4_l4') or i in set(sample):
            want = ref.qhull(E, f)
            assert ref.same_set(V, want, tol=1e-6), (i, len(V), len(want))
            checked += 1
    assert checked > 0 and numpy.count_nonzero(rv.status == OK) >= 0.99 * n_reg, rv.stats


def test_determinism():
    sol = _solve('c3_l4')
    ef, row_off, _ = sol._stacked()
    from ppopt_amd.geometry.vertices import vertices_of_rows
    a = vertices_of_rows(row_off, ef, ef.shape[1] - 1)
    b = vertices_of_rows(row_off, ef, ef.shape[1] - 1)
    for k in ('vertices', 'offsets', 'incidence', 'rays', 'ray_offsets', 'status'):
        assert numpy.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.vertices.tobytes() == b.vertices.tobytes()
