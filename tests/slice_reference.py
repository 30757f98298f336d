"""An independent CPU reference for the 2-D and 1-D slices of polytopes (mpc_slice_polygons / mpc_slice_intervals).  It shares no
code with the kernel or the package: scipy's linprog decides feasibility and gives the Chebyshev radius, HalfspaceIntersection and
ConvexHull give the vertices and the area, and an edge's rows are the rows with zero slack at the edge's midpoint."""
import numpy
from scipy.optimize import linprog
from scipy.spatial import ConvexHull, HalfspaceIntersection

FULL, EMPTY, LOWDIM, CUT = 0, 1, 2, 4


def reduce_rows(E, f, theta_0, U, box, eps=1e-9):
    """Rows (a [k, 2], beta [k], ids [k]) of the slice in coordinates about the box centre, normalised, rows constant on the plane
    dropped, the four box rows appended with ids -1 .. -4; and whether a constant row excludes the whole plane."""
    E = numpy.asarray(E, dtype=float).reshape(len(f), -1)
    f = numpy.asarray(f, dtype=float).reshape(-1)
    U = numpy.asarray(U, dtype=float)
    lo0, lo1, hi0, hi1 = (float(v) for v in box)
    c = numpy.array([(lo0 + hi0) / 2, (lo1 + hi1) / 2])
    hx, hy = (hi0 - lo0) / 2, (hi1 - lo1) / 2
    th_c = numpy.asarray(theta_0, dtype=float) + U @ c
    A = E @ U
    dot = E @ th_c
    beta = f - dot
    nrm = numpy.linalg.norm(A, axis=1)
    const = nrm <= eps * numpy.linalg.norm(E, axis=1) * numpy.max(numpy.linalg.norm(U, axis=0))
    violated = bool(numpy.any(const & (beta < -eps * (numpy.abs(f) + numpy.abs(dot)))))
    keep = ~const
    a = A[keep] / nrm[keep, None]
    b = beta[keep] / nrm[keep]
    ids = numpy.flatnonzero(keep)
    a = numpy.vstack([a, [[1, 0], [0, 1], [-1, 0], [0, -1]]])
    b = numpy.concatenate([b, [hx, hy, hx, hy]])
    ids = numpy.concatenate([ids, [-1, -2, -3, -4]])
    return a, b, ids, c, violated


def sort_ccw(V):
    """Ascending atan2 about the mean (the reference's sort_clockwise order)."""
    m = V.mean(axis=0)
    return V[numpy.argsort(numpy.arctan2(V[:, 1] - m[1], V[:, 0] - m[0]), kind='stable')]


def slice_polygon(E, f, theta_0, U, box, eps=1e-9, lowdim_radius=1e-7):
    """dict(status, vertices [k, 2] (z, ascending atan2 about their mean), area, edge_rows: for every vertex the set of row ids with
    zero slack at the midpoint of the edge that starts there, radius)."""
    a, b, ids, c, violated = reduce_rows(E, f, theta_0, U, box, eps)
    D = 2 * numpy.hypot((box[2] - box[0]) / 2, (box[3] - box[1]) / 2)
    out = dict(status=EMPTY, vertices=numpy.zeros((0, 2)), area=0.0, edge_rows=[], radius=numpy.nan)
    if violated:
        return out
    # Chebyshev ball: max r s.t. a_i z + r <= b_i (|a_i| = 1)
    res = linprog([0, 0, -1], A_ub=numpy.hstack([a, numpy.ones((len(b), 1))]), b_ub=b, bounds=[(None, None), (None, None), (0, None)],
                  method='highs')
    if res.status == 2:
        return out
    assert res.status == 0, res.message
    r = res.x[2]
    out['radius'] = r
    if r <= lowdim_radius * D:
        out['status'] = LOWDIM
        return out
    hs = HalfspaceIntersection(numpy.hstack([a, -b[:, None]]), res.x[:2])
    hull = ConvexHull(hs.intersections)
    V = hs.intersections[hull.vertices]
    keep = []
    for v in V:                                    # points Qhull did not merge
        if not any(numpy.max(numpy.abs(v - w)) <= 1e-12 * D for w in keep):
            keep.append(v)
    V = sort_ccw(numpy.array(keep))
    edges = []
    for k in range(len(V)):
        mid = (V[k] + V[(k + 1) % len(V)]) / 2
        slack = b - a @ mid
        edges.append(set(int(i) for i in ids[numpy.abs(slack) <= 1e-9 * D]))
    out.update(status=FULL | (CUT if any(all(i < 0 for i in e) for e in edges) else 0), vertices=V + c, area=float(hull.volume),
               edge_rows=edges)
    return out


def slice_interval(E, f, theta_0, u, t_range, eps=1e-9):
    """(t_a, t_b, status) of {t : E (theta_0 + u t) <= f} within t_range, by two LPs (NaN, NaN, EMPTY when it is empty)."""
    E = numpy.asarray(E, dtype=float).reshape(len(f), -1)
    f = numpy.asarray(f, dtype=float).reshape(-1)
    a, dot = E @ numpy.asarray(u, dtype=float), E @ numpy.asarray(theta_0, dtype=float)
    beta = f - dot
    const = numpy.abs(a) <= eps * numpy.linalg.norm(E, axis=1) * numpy.linalg.norm(u)
    if numpy.any(const & (beta < -eps * (numpy.abs(f) + numpy.abs(dot)))):
        return numpy.nan, numpy.nan, EMPTY
    A, b = a[~const, None], beta[~const]
    lo = linprog([1], A_ub=A if len(b) else None, b_ub=b if len(b) else None, bounds=[t_range], method='highs')
    if lo.status == 2:
        return numpy.nan, numpy.nan, EMPTY
    hi = linprog([-1], A_ub=A if len(b) else None, b_ub=b if len(b) else None, bounds=[t_range], method='highs')
    ta, tb = lo.x[0], hi.x[0]
    L = t_range[1] - t_range[0]
    st = LOWDIM if tb - ta <= eps * L else FULL
    if numpy.isclose(ta, t_range[0], rtol=0, atol=1e-12 * L) or numpy.isclose(tb, t_range[1], rtol=0, atol=1e-12 * L):
        st |= CUT
    return ta, tb, st
