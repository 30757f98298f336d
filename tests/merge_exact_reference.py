"""An exact check of merged regions that does not depend on the merge rules: numpy and scipy.optimize.linprog (HiGHS)
only, no package code.

    chebyshev_radius(E, f)                      radius of the largest ball in {E theta <= f}; -inf when empty, +inf when unbounded
    difference_radius(E, f, others, tol)        the largest Chebyshev radius of a piece of {E theta <= f} minus the union of ``others``
                                                (a list of (E, f)); 0.0 when nothing fatter than tol is left
    union_defect(U, members, tol)               (outside, missing): difference_radius(U, members) and the largest
                                                difference_radius(member, [U])

The difference is the usual region-difference recursion: for the first other polytope with rows 1..k, P minus it is the disjoint union
of P n {row_1 reversed}, P n {row_1} n {row_2 reversed}, ..., each of which goes on against the rest.  An other polytope whose
intersection with P has radius <= tol is skipped, and a branch whose radius is <= tol ends.
"""
import numpy
from scipy.optimize import linprog


# HiGHS's default feasibility tolerances (1e-7) let a vertex between nearly parallel rows violate them by 3e-8 and move a radius by 1e-8,
# the size of what is measured here; at 1e-10 its radii agree with the device's to 1e-14
_HIGHS = {'primal_feasibility_tolerance': 1e-10, 'dual_feasibility_tolerance': 1e-10}


def _rows(E, f):
    E = numpy.asarray(E, dtype=float)
    f = numpy.asarray(f, dtype=float).reshape(-1)
    return E.reshape(len(f), -1), f


def chebyshev_radius(E, f):
    """max r s.t. E theta + |E_i| r <= f; -inf when {E theta <= f} is empty, +inf when the ball is unbounded"""
    E, f = _rows(E, f)
    n = E.shape[1]
    nrm = numpy.linalg.norm(E, axis=1)
    if numpy.any((nrm == 0.0) & (f < 0.0)):
        return -numpy.inf
    keep = nrm > 0.0
    c = numpy.zeros(n + 1)
    c[n] = -1.0
    r = linprog(c, A_ub=numpy.column_stack([E[keep], nrm[keep]]), b_ub=f[keep], bounds=[(None, None)] * (n + 1), method='highs',
                options=_HIGHS)
    if r.status == 3:
        return numpy.inf
    if r.status != 0:
        return -numpy.inf
    return float(-r.fun)


def difference_radius(E, f, others, tol=1e-8):
    E, f = _rows(E, f)
    r = chebyshev_radius(E, f)
    if not r > tol:
        return 0.0
    for k, (Eo, fo) in enumerate(others):
        Eo, fo = _rows(Eo, fo)
        if not chebyshev_radius(numpy.vstack([E, Eo]), numpy.concatenate([f, fo])) > tol:
            continue
        best = 0.0
        Ec, fc = E, f
        for i in range(len(fo)):
            best = max(best, difference_radius(numpy.vstack([Ec, -Eo[i:i + 1]]), numpy.append(fc, -fo[i]), others[k + 1:], tol))
            Ec, fc = numpy.vstack([Ec, Eo[i:i + 1]]), numpy.append(fc, fo[i])
        return best
    return r


def union_defect(U, members, tol=1e-8):
    """(outside, missing) of a claimed union U = (E, f) of ``members`` (a list of (E, f))"""
    outside = difference_radius(U[0], U[1], list(members), tol)
    missing = max([difference_radius(E, f, [U], tol) for E, f in members], default=0.0)
    return outside, missing
