"""Vertex sets of polytopes {x : A x <= b} without the device kernel: a brute force over every n-subset of rows, and
scipy's HalfspaceIntersection from the Chebyshev centre, both deduplicated; plus known polytopes with their vertex sets."""
import itertools

import numpy


def dedupe(V, tol=1e-7):
    """rows of V with near-duplicates (max-norm <= tol (1 + |v|)) removed, in lexicographic order"""
    V = numpy.atleast_2d(numpy.asarray(V, dtype=float))
    out = []
    for v in V[numpy.lexsort(V.T[::-1])]:
        if not any(numpy.max(numpy.abs(v - w)) <= tol * (1 + numpy.max(numpy.abs(v))) for w in out):
            out.append(v)
    return numpy.array(out).reshape(len(out), V.shape[1])


def brute_force(A, b, tol=1e-9):
    """every feasible solution of n tight rows with a nonsingular n x n system, deduplicated (small row counts only)"""
    A, b = numpy.asarray(A, dtype=float), numpy.asarray(b, dtype=float).reshape(-1)
    m, n = A.shape
    pts = []
    for rows in itertools.combinations(range(m), n):
        M = A[list(rows)]
        if abs(numpy.linalg.det(M)) < 1e-12 * max(1.0, numpy.max(numpy.abs(M)) ** n):
            continue
        v = numpy.linalg.solve(M, b[list(rows)])
        if numpy.all(A @ v <= b + tol * (1 + numpy.abs(b))):
            pts.append(v)
    return dedupe(numpy.array(pts).reshape(-1, n))


def chebyshev_centre(A, b):
    from scipy.optimize import linprog
    A, b = numpy.asarray(A, dtype=float), numpy.asarray(b, dtype=float).reshape(-1)
    n = A.shape[1]
    norm = numpy.linalg.norm(A, axis=1)
    res = linprog(numpy.r_[numpy.zeros(n), -1.0], A_ub=numpy.c_[A, norm], b_ub=b, bounds=[(None, None)] * n + [(0, None)], method='highs')
    return res.x[:n], res.x[n]


def qhull(A, b):
    """scipy.spatial.HalfspaceIntersection from the Chebyshev centre, deduplicated (bounded, full-dimensional polytopes)"""
    from scipy.spatial import HalfspaceIntersection
    A, b = numpy.asarray(A, dtype=float), numpy.asarray(b, dtype=float).reshape(-1)
    c, _ = chebyshev_centre(A, b)
    hs = HalfspaceIntersection(numpy.c_[A, -b], c)
    return dedupe(hs.intersections)


def same_set(V, W, tol=1e-6):
    """equal counts and every point of V within tol (1 + |v|) of a point of W"""
    V, W = numpy.asarray(V, dtype=float), numpy.asarray(W, dtype=float)
    if len(V) != len(W):
        return False
    for v in V:
        if numpy.min(numpy.max(numpy.abs(W - v), axis=1)) > tol * (1 + numpy.max(numpy.abs(v))):
            return False
    return True


# ---- known polytopes --------------------------------------------------------------------------------------------------------------
def cube(n):
    return numpy.vstack([numpy.eye(n), -numpy.eye(n)]), numpy.ones(2 * n), numpy.array(list(itertools.product((-1.0, 1.0), repeat=n)))


def simplex(n):
    """{x >= 0, sum x <= 1}"""
    A = numpy.vstack([-numpy.eye(n), numpy.ones((1, n))])
    return A, numpy.r_[numpy.zeros(n), 1.0], numpy.vstack([numpy.zeros(n), numpy.eye(n)])


def cross_polytope(n):
    """{x : s.x <= 1 for every sign vector s}: 2^n facets, 2n vertices +-e_i, 2^(n-1) facets meet at each vertex"""
    S = numpy.array(list(itertools.product((-1.0, 1.0), repeat=n)))
    return S, numpy.ones(len(S)), numpy.vstack([numpy.eye(n), -numpy.eye(n)])


def cyclic_polytope(n, k):
    """the convex hull of k points on the moment curve (t, t^2, ..., t^n): every point is a vertex; H-representation by qhull"""
    from scipy.spatial import ConvexHull
    t = numpy.linspace(-1.0, 1.0, k)
    P = numpy.stack([t ** (j + 1) for j in range(n)], axis=1)
    hull = ConvexHull(P)
    eq = hull.equations
    return eq[:, :-1], -eq[:, -1], P
