"""The numpy restatement of the volume recursion (tests/volume_reference.py) against closed forms and qhull, and its
simplex counts; no device."""
import math

import numpy
import pytest

import vertex_reference as vref
import volume_reference as ref


def _random(rng, n, cuts):
    """a scaled, shifted simplex cut by random rows through its interior (the generator of test_gpu_vertices)"""
    A, b, _ = vref.simplex(n)
    c = rng.normal(size=n)
    A = numpy.vstack([A, rng.normal(size=(cuts, n))])
    x0 = numpy.full(n, 1.0 / (n + 1))
    b = numpy.r_[b, A[n + 1:] @ x0 + rng.uniform(0.01, 0.2, size=cuts)]
    s = rng.uniform(0.5, 3.0)
    return A, s * b + A @ c


@pytest.mark.parametrize('n', range(2, 8))
def test_cube(n):
    A, b, V = vref.cube(n)
    vol, cen, count = ref.reference(A, b, V)
    assert abs(vol - 2.0 ** n) <= 1e-12 * 2.0 ** n
    assert numpy.max(numpy.abs(cen)) <= 1e-12
    assert count == math.factorial(n)          # n facets avoid the apex, each an (n - 1)-cube: n (n - 1) ... 1


@pytest.mark.parametrize('n', range(2, 8))
def test_simplex(n):
    A, b, V = vref.simplex(n)
    vol, cen, count = ref.reference(A, b, V)
    assert abs(vol - 1.0 / math.factorial(n)) <= 1e-12 / math.factorial(n)
    assert numpy.max(numpy.abs(cen - 1.0 / (n + 1))) <= 1e-12
    assert count == 1


@pytest.mark.parametrize('n', range(3, 7))
def test_cross_polytope(n):
    A, b, V = vref.cross_polytope(n)
    vol, cen, _ = ref.reference(A, b, V)
    assert abs(vol - 2.0 ** n / math.factorial(n)) <= 1e-12 * 2.0 ** n / math.factorial(n)
    assert numpy.max(numpy.abs(cen)) <= 1e-12


@pytest.mark.parametrize('n', range(2, 7))
def test_random_against_qhull(n):
    rng = numpy.random.default_rng(n)
    for _ in range(4):
        A, b = _random(rng, n, 6)
        V = vref.qhull(A, b)
        vol, cen, _ = ref.reference(A, b, V)
        want = ref.qhull_volume(V)
        assert abs(vol - want) <= 1e-12 * want, (vol, want)
        assert numpy.all(A @ cen <= b)


def test_blurred_incidence_is_refused():
    A, b, V = vref.cube(3)
    V = ref.sort_vertices(V)
    C = ref.row_sets(A, b, V)
    C[1] = C[1] | {5}                        # (1, -1, 1) claimed by the facet x_1 = 1: an edge of three vertices
    with pytest.raises(ValueError):
        ref.triangulate(V, C)
