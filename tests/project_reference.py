"""An independent CPU statement of the projection rule of DESIGN §3.24 (numpy and scipy's HiGHS): the same definition, thresholds and
order as ppopt_amd/geometry/project.py and csrc/project.hpp, none of their code.

  project_one(rows, n_elim, tol, out_cap)  -> a ReferenceProjection of one polytope of unit rows [o | n]: its trailing n_elim coordinates
                                              are eliminated, the last one first.  status, rows (the result, in order), wide (the runs
                                              that came back unbounded, which keep their row), peak, lp (every LP value in the order of
                                              the runs, +inf where unbounded), nu (the smallest nonzero combination norm before scaling,
                                              +inf without one), knife.
  eliminate(rows, tol)                     -> one step without its reduce: (new rows, |Z| + |P||N|, empty, nu)
  radius(rows)                             -> (unbounded, r): the largest t with n.x + t <= o over the rows, x and t free

A decision is a KNIFE decision when its reference radius lies within KNIFE of tol: HiGHS answers within its own 1e-7, and the device,
whose simplex rounds otherwise, may legitimately decide there the other way.  A polytope with a knife decision is a knife polytope and is
not compared row by row.  The comparisons run at tol = 1e-6, so an exact-zero radius (duplicates, touching rows) lies far outside the band.
"""
from dataclasses import dataclass, field

import numpy
from scipy.optimize import linprog

KNIFE = 5e-7
ZERO_COEF, ZERO_NORM, MAX_ROWS = 1e-12, 1e-9, 512
OK, THIN, WHOLE, TOO_LARGE = range(4)


@dataclass
class ReferenceProjection:
    status: int
    rows: numpy.ndarray
    wide: int
    peak: int
    lp: list = field(default_factory=list)
    nu: float = numpy.inf
    knife: bool = False


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


def eliminate(rows, tol):
    rows = numpy.asarray(rows, dtype=float)
    d = rows.shape[1] - 1                      # column d holds coordinate j = d - 1
    c = rows[:, d]
    P, N = numpy.flatnonzero(c > ZERO_COEF), numpy.flatnonzero(c < -ZERO_COEF)
    Z = numpy.flatnonzero(numpy.abs(c) <= ZERO_COEF)
    new, empty, nu = [], False, numpy.inf
    for i in Z:
        v = rows[i, :d].copy()
        if c[i] != 0.0:
            v /= numpy.linalg.norm(v[1:])
        new.append(v)
    pairs = len(P) * len(N)
    for p in P:
        for q in N:
            v = (-c[q]) * rows[p, :d] + c[p] * rows[q, :d]
            nrm = float(numpy.linalg.norm(v[1:]))
            if nrm <= ZERO_NORM:
                empty = empty or v[0] < -tol
                continue
            nu = min(nu, nrm)
            new.append(v / nrm)
    return (numpy.array(new) if new else numpy.zeros((0, d))), len(Z) + pairs, empty, nu


def _reduce(rows, tol, out):
    """the sequential rule of §3.22 over rows, started after a thin test that passed: the kept rows"""
    kept = numpy.ones(len(rows), dtype=bool)
    for k in range(len(rows)):
        live = kept.copy()
        live[k] = False
        open_k, rk = radius(numpy.vstack([rows[live], -rows[k][None]]))
        out.lp.append(rk)
        if open_k:
            out.wide += 1
            continue
        out.knife = out.knife or abs(rk - tol) <= KNIFE
        if not rk > tol:
            kept[k] = False
    return rows[kept]


def _thin(rows, tol, out):
    open_, r = radius(rows)
    out.lp.append(r)
    out.wide += int(open_)
    out.knife = out.knife or ((not open_) and abs(r - tol) <= KNIFE)
    return (not open_) and not r > tol


def project_one(rows, n_elim, tol=1e-6, out_cap=MAX_ROWS):
    live = numpy.asarray(rows, dtype=float)
    n = live.shape[1] - 1
    out = ReferenceProjection(OK, numpy.zeros((0, n - n_elim + 1)), 0, 0)

    def end(status):
        out.status = status
        return out

    if _thin(live, tol, out):
        return end(THIN)
    if n_elim == 0:
        live = _reduce(live, tol, out)
    for _ in range(n_elim):
        live, total, empty, nu = eliminate(live, tol)
        out.peak, out.nu = max(out.peak, total), min(out.nu, nu)
        if total > MAX_ROWS:
            return end(TOO_LARGE)
        if empty:
            return end(THIN)
        if not len(live):
            return end(WHOLE)
        if _thin(live, tol, out):
            return end(THIN)
        live = _reduce(live, tol, out)
    if len(live) > out_cap:
        return end(TOO_LARGE)
    out.rows = live
    return out


def project_reference(polys, n_elim, tol=1e-6, out_cap=MAX_ROWS):
    return [project_one(p, n_elim, tol, out_cap) for p in polys]


def support(rows, direction):
    """max direction.x over {x : n.x <= o}: +inf when unbounded"""
    rows = numpy.asarray(rows, dtype=float)
    res = linprog(-numpy.asarray(direction, dtype=float), A_ub=rows[:, 1:], b_ub=rows[:, 0], bounds=[(None, None)] * (rows.shape[1] - 1),
                  method='highs')
    if res.status == 0:
        return -float(res.fun)
    if res.status in (3, 4):
        return numpy.inf
    raise RuntimeError(f'the support LP ended with status {res.status}: {res.message}')
