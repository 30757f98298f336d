"""An independent CPU statement of the sequential rule of DESIGN §3.22 (numpy and scipy's HiGHS): the same definition, thresholds and
order as ppopt_amd/geometry/reduce.py and csrc/reduce.hpp, none of their code.

  reduce_reference(polys, tol)  -> one ReferenceResult per polytope (unit rows [o | n]): kept [m] bool, thin, wide (the runs that came
                                   back unbounded, which keep their row), radius (of P), row_radius [m] (the radius of every row's run,
                                   NaN where none ran, +inf where unbounded), knife.
  radius(rows)                  -> (unbounded, r): the largest t with n.theta + t <= o over the rows, theta and t free

A decision is a KNIFE decision when its reference radius lies within KNIFE of tol: HiGHS answers within its own 1e-7, and the device,
whose simplex rounds otherwise, may legitimately decide there the other way.  A polytope with a knife decision is a knife polytope and is
not compared row by row.  The comparisons run at tol = 1e-6, so an exact-zero radius (duplicates, touching rows) lies far outside the band.
"""
from dataclasses import dataclass

import numpy
from scipy.optimize import linprog

KNIFE = 5e-7


@dataclass
class ReferenceResult:
    kept: numpy.ndarray
    thin: bool
    wide: int
    radius: float
    row_radius: numpy.ndarray
    knife: bool


def radius(rows):
    rows = numpy.asarray(rows, dtype=float)
    n = rows.shape[1] - 1
    c = numpy.append(numpy.zeros(n), -1.0)
    A = numpy.hstack([rows[:, 1:], numpy.ones((len(rows), 1))])
    res = linprog(c, A_ub=A, b_ub=rows[:, 0], bounds=[(None, None)] * (n + 1), method='highs')
    if res.status == 0:
        return False, -float(res.fun)
    if res.status == 3:
        return True, numpy.inf
    # "unbounded or infeasible" cannot be infeasible (t is free below): bound t and look at where the optimum lands
    res = linprog(c, A_ub=A, b_ub=rows[:, 0], bounds=[(None, None)] * n + [(None, 1e6)], method='highs')
    if res.status == 0:
        r = -float(res.fun)
        return (True, numpy.inf) if r >= 1e6 * (1 - 1e-9) else (False, r)
    raise RuntimeError(f'the radius LP ended with status {res.status}: {res.message}')


def reduce_one(rows, tol):
    rows = numpy.asarray(rows, dtype=float)
    m = len(rows)
    kept = numpy.ones(m, dtype=bool)
    row_radius = numpy.full(m, numpy.nan)
    open_, r = radius(rows)
    knife = (not open_) and abs(r - tol) <= KNIFE
    wide = int(open_)
    if not open_ and not r > tol:
        return ReferenceResult(kept, True, 0, r, row_radius, knife)
    for k in range(m):
        live = kept.copy()
        live[k] = False
        open_k, rk = radius(numpy.vstack([rows[live], -rows[k][None]]))
        row_radius[k] = rk
        if open_k:
            wide += 1
            continue
        knife = knife or abs(rk - tol) <= KNIFE
        if not rk > tol:
            kept[k] = False
    return ReferenceResult(kept, False, wide, r, row_radius, knife)


def reduce_reference(polys, tol=1e-6):
    return [reduce_one(p, tol) for p in polys]
