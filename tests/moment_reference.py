"""Second moments of polytopes without the device kernel: the exact simplex formula
    int_D theta theta^T = |D| / ((n + 1)(n + 2)) (sum_i v_i v_i^T + s s^T),  s = sum_i v_i,
summed over the simplices of tests/volume_reference.triangulate (the recursion of csrc/volume.hpp in numpy) and over those of scipy's
Delaunay triangulation of the same vertices."""
import math

import numpy

import volume_reference as ref


def simplex_moments(P):
    """(M0, M1 [n], M2 [n, n]) of the simplex with the vertices P [n + 1, n]"""
    P = numpy.asarray(P, dtype=float)
    n = P.shape[1]
    vol = abs(numpy.linalg.det(P[1:] - P[0])) / math.factorial(n)
    s = P.sum(axis=0)
    return vol, vol * s / (n + 1), vol / ((n + 1) * (n + 2)) * (P.T @ P + numpy.outer(s, s))


def _sum(V, simplices):
    n = V.shape[1]
    m0, m1, m2 = 0.0, numpy.zeros(n), numpy.zeros((n, n))
    for s in simplices:
        a, b, c = simplex_moments(V[list(s)])
        m0, m1, m2 = m0 + a, m1 + b, m2 + c
    return m0, m1, m2


def reference_moments(A, b, V, tol=1e-9):
    """(M0, M1, M2) of {x : A x <= b} with the vertices V, on the simplices of volume_reference.triangulate"""
    V = ref.sort_vertices(V)
    return _sum(V, ref.triangulate(V, ref.row_sets(A, b, V, tol))[2])


def delaunay_moments(V):
    """(M0, M1, M2) of the convex hull of V on qhull's Delaunay triangulation; for n <= 5 (beyond, qhull drops slivers)"""
    from scipy.spatial import Delaunay
    V = numpy.atleast_2d(numpy.asarray(V, dtype=float))
    assert V.shape[1] <= 5
    return _sum(V, Delaunay(V).simplices)


def cube_m2(n):
    return 2.0 ** n / 3.0 * numpy.eye(n)


def simplex_m2(n):
    return (1.0 + numpy.eye(n)) / math.factorial(n + 2)


def cross_m2(n):
    return 2.0 ** n * 2.0 / math.factorial(n + 2) * numpy.eye(n)
