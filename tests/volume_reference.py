"""Volumes and centroids of polytopes without the device kernel: the boundary triangulation of Cohen & Hickey restated in
numpy on frozensets (the recursion of csrc/volume.hpp, with numpy.linalg.det for the simplices), and scipy's ConvexHull volume."""
import math

import numpy

import vertex_reference as vref


def sort_vertices(V):
    V = numpy.atleast_2d(numpy.asarray(V, dtype=float))
    return V[numpy.lexsort(V.T[::-1])]


def row_sets(A, b, V, tol=1e-9):
    """C_r: the vertices (indices into V) tight on row r, |b_r - a_r v| <= tol (1 + |b_r|)"""
    A, b = numpy.asarray(A, dtype=float), numpy.asarray(b, dtype=float).reshape(-1)
    tight = numpy.abs(b[None] - V @ A.T) <= tol * (1 + numpy.abs(b))[None]
    return [frozenset(numpy.flatnonzero(tight[:, r]).tolist()) for r in range(len(b))]


def facets(S, C):
    """the maximal proper non-empty sets among {S & C_r}, equal sets once, in the order of their lowest row"""
    cand = []
    for c in C:
        T = S & c
        if T and T != S and T not in cand:
            cand.append(T)
    return [T for T in cand if not any(T < U for U in cand)]


def triangulate(V, C):
    """(volume, centroid, simplices): V [k, n] in the order that names the apexes, C the row sets.  simplices is the list of vertex index
    tuples (chain, then the last vertex).  ValueError where the sets are no face lattice."""
    V = numpy.asarray(V, dtype=float)
    n = V.shape[1]
    out = []

    def walk(S, d, chain):
        if d == 0:
            if len(S) != 1:
                raise ValueError(f'a face of dimension 0 holds {len(S)} vertices')
            out.append(tuple(chain) + tuple(S))
            return
        apex = min(S)
        F = facets(S, C)
        if not F:
            raise ValueError(f'a face of dimension {d} has no facet')
        for T in F:
            if apex not in T:
                walk(T, d - 1, chain + [apex])

    walk(frozenset(range(len(V))), n, [])
    vol, mom = 0.0, numpy.zeros(n)
    for s in out:
        P = V[list(s)]
        v = abs(numpy.linalg.det(P[1:] - P[0])) / math.factorial(n)
        vol += v
        mom += v * P.mean(axis=0)
    return vol, mom / vol, out


def reference(A, b, V=None, tol=1e-9):
    """(volume, centroid, simplex count) of {x : A x <= b}; V: its vertices (None: vertex_reference.qhull), sorted lexicographically here"""
    V = sort_vertices(vref.qhull(A, b) if V is None else V)
    vol, cen, simplices = triangulate(V, row_sets(A, b, V, tol))
    return vol, cen, len(simplices)


def qhull_volume(V):
    """the volume of the convex hull of the points V by qhull: scipy's ConvexHull; where qhull gives up on the hull with a precision
    error (nearly coplanar facets), the summed simplex volumes of qhull's Delaunay triangulation of the same points"""
    from scipy.spatial import ConvexHull, Delaunay, QhullError
    V = numpy.atleast_2d(numpy.asarray(V, dtype=float))
    n = V.shape[1]
    if n == 1:
        return float(V.max() - V.min())
    try:
        return float(ConvexHull(V).volume)
    except QhullError:
        return float(sum(abs(numpy.linalg.det(V[s[1:]] - V[s[0]])) for s in Delaunay(V).simplices) / math.factorial(n))
