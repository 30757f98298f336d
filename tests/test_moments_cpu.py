"""The second-moment references of tests/moment_reference.py against closed forms and against each other, and the host
algebra of geometry.moments (value_function, integrate_quadratic, first_moment, covariance); no device.

Bound: 1e-13 relative to the largest entry of the reference (3.2e-15 observed)."""
import numpy
import pytest

import moment_reference as mref
import vertex_reference as vref
from ppopt_amd import CriticalRegion, MPLP_Program, MPQP_Program, Solution
from ppopt_amd.geometry.moments import RegionMoments, integrate_quadratic
from test_volume_cpu import _random

RTOL = 1e-13
OK, UNBOUNDED, EMPTY, TOO_LARGE = 0, 1, 3, 5


def _close(got, want):
    got, want = numpy.asarray(got, dtype=float), numpy.asarray(want, dtype=float)
    d = numpy.max(numpy.abs(got - want)) / numpy.max(numpy.abs(want))
    print(f'relative difference {d:.3e}')
    return d <= RTOL


KNOWN = [('cube', n, vref.cube, mref.cube_m2) for n in range(2, 7)] + [('simplex', n, vref.simplex, mref.simplex_m2) for n in range(2, 7)] + \
        [('cross', n, vref.cross_polytope, mref.cross_m2) for n in range(2, 7)]


@pytest.mark.parametrize('name,n,make,m2', KNOWN, ids=[f'{k[0]}{k[1]}' for k in KNOWN])
def test_references_against_closed_forms(name, n, make, m2):
    A, b, V = make(n)
    assert _close(mref.reference_moments(A, b, V)[2], m2(n))
    if n <= 5:
        assert _close(mref.delaunay_moments(V)[2], m2(n))


@pytest.mark.parametrize('n', [2, 3, 5])
def test_references_against_each_other(n):
    rng = numpy.random.default_rng(n)
    for _ in range(4):
        A, b = _random(rng, n, 6)
        V = vref.qhull(A, b)
        r0, r1, r2 = mref.reference_moments(A, b, V)
        d0, d1, d2 = mref.delaunay_moments(V)
        assert abs(r0 - d0) <= RTOL * d0 and _close(r1, d1) and _close(r2, d2)


class _Prog:
    """the objective terms of a program without its constructor; evaluate_objective is the program class's own"""

    def __init__(self, cls, rng, n_x, n_t):
        L = rng.normal(size=(n_x, n_x))
        self.Q = L @ L.T + numpy.eye(n_x)
        self.H, self.c, self.c_t = rng.normal(size=(n_x, n_t)), rng.normal(size=(n_x, 1)), rng.normal(size=(n_t, 1))
        S = rng.normal(size=(n_t, n_t))
        self.Q_t, self.c_c = S + S.T, rng.normal(size=(1, 1))
        self.n_t, self.cls = n_t, cls
        if cls is MPLP_Program:
            del self.Q

    def num_t(self):
        return self.n_t

    def evaluate_objective(self, x, theta):
        return self.cls.evaluate_objective(self, x, theta)


@pytest.mark.parametrize('cls', [MPQP_Program, MPLP_Program])
def test_value_function(cls):
    rng = numpy.random.default_rng(7)
    n_x, n_t, R = 4, 3, 5
    prog = _Prog(cls, rng, n_x, n_t)
    E, f = numpy.vstack([numpy.eye(n_t), -numpy.eye(n_t)]), numpy.ones((2 * n_t, 1))
    regs = [CriticalRegion(rng.normal(size=(n_x, n_t)), rng.normal(size=(n_x, 1)), numpy.zeros((1, n_t)), numpy.zeros((1, 1)), E, f, [0], [], [])
            for _ in range(R)]
    sol = Solution(prog, regs)
    Qv, qv, rv = sol.value_function()
    assert Qv.shape == (R, n_t, n_t) and qv.shape == (R, n_t) and rv.shape == (R,)
    for i, cr in enumerate(regs):
        for _ in range(4):
            th = rng.uniform(-1, 1, size=(n_t, 1))
            want = prog.evaluate_objective(cr.evaluate(th), th)
            got = 0.5 * th[:, 0] @ Qv[i] @ th[:, 0] + qv[i] @ th[:, 0] + rv[i]
            assert abs(got - want) <= RTOL * max(1.0, abs(want))


def _moments():
    """a unit square [0, 1]^2, the triangle of the unit simplex, an empty set, an unbounded one and one over the work cap, by hand"""
    nan = numpy.nan
    m2 = numpy.array([[[1 / 3, 1 / 4], [1 / 4, 1 / 3]], mref.simplex_m2(2), numpy.zeros((2, 2)), numpy.full((2, 2), nan), numpy.full((2, 2), nan)])
    return RegionMoments(volume=numpy.array([1.0, 0.5, 0.0, numpy.inf, nan]), centroid=numpy.array([[0.5, 0.5], [1 / 3, 1 / 3], [nan, nan], [nan, nan], [nan, nan]]),
                         second_moment=m2, simplices=numpy.array([2, 1, 0, 0, 0]), status=numpy.array([OK, OK, EMPTY, UNBOUNDED, TOO_LARGE], dtype=numpy.int32))


def test_integrate_quadratic():
    mom = _moments()
    rng = numpy.random.default_rng(3)
    Q, q, r = rng.normal(size=(2, 2)), rng.normal(size=2), 0.7
    # the definition on the square by Gauss-Legendre (exact for a quadratic), on the triangle by the three edge midpoints
    g, w = numpy.polynomial.legendre.leggauss(3)
    g, w = 0.5 * (g + 1), 0.5 * w
    fun = lambda x, y, Q, q, r: 0.5 * (Q[0, 0] * x * x + (Q[0, 1] + Q[1, 0]) * x * y + Q[1, 1] * y * y) + q[0] * x + q[1] * y + r
    square = lambda Q, q, r: sum(wi * wj * fun(gi, gj, Q, q, r) for gi, wi in zip(g, w) for gj, wj in zip(g, w))
    triangle = lambda Q, q, r: sum(fun(x, y, Q, q, r) for x, y in ((0.5, 0), (0, 0.5), (0.5, 0.5))) / 6
    out = integrate_quadratic(mom, Q, q, r)
    assert _close(out[:2], [square(Q, q, r), triangle(Q, q, r)])
    assert out[2] == 0.0 and numpy.isnan(out[3:]).all()
    # per polytope coefficients, and every coefficient on its own
    Qs, qs, rs = rng.normal(size=(5, 2, 2)), rng.normal(size=(5, 2)), rng.normal(size=5)
    out = integrate_quadratic(mom, Qs, qs, rs)
    assert _close(out[:2], [square(Qs[0], qs[0], rs[0]), triangle(Qs[1], qs[1], rs[1])]) and out[2] == 0.0 and numpy.isnan(out[3:]).all()
    zQ, zq = numpy.zeros((2, 2)), numpy.zeros(2)
    assert _close(integrate_quadratic(mom, Q=Q)[:2], [square(Q, zq, 0), triangle(Q, zq, 0)])
    assert _close(integrate_quadratic(mom, q=q)[:2], [square(zQ, q, 0), triangle(zQ, q, 0)])
    assert integrate_quadratic(mom, r=1.0)[:3].tolist() == [1.0, 0.5, 0.0]
    with pytest.raises(ValueError, match='shape'):
        integrate_quadratic(mom, Q=numpy.zeros((3, 3)))


def test_first_moment_and_covariance():
    mom = _moments()
    m1, cov = mom.first_moment, mom.covariance
    assert _close(m1[:2], [[0.5, 0.5], [1 / 6, 1 / 6]]) and m1[2].tolist() == [0.0, 0.0] and numpy.isnan(m1[3:]).all()
    assert _close(cov[0], numpy.eye(2) / 12) and _close(cov[1], numpy.array([[2, -1], [-1, 2]]) / 36.0)
    assert numpy.isnan(cov[2:]).all()
