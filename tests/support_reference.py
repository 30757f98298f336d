"""An independent CPU statement of the support function of DESIGN §3.28 and of what is built on it (numpy and scipy's HiGHS): the same
definitions as ppopt_amd/geometry/support.py and csrc/support.hpp, none of their code.

  radius(rows)                 -> (unbounded, r, theta): the largest t with n.theta + t <= o over the unit rows, theta and t free
  support(rows, d)             -> (status, value, arg): max d.x over the rows; status 0: optimal, 3: unbounded (value +inf, arg None)
  erosion(p_rows, q_rows, E)   -> (empty, rows): the rows [o_k - h_Q(E' n_k) | n_k]; empty when some h_k is +inf (rows None)
  containment(inner, outer)    -> (excess, row, witness): max_k (h_inner(n_k) - o_k) over the rows of outer, the lowest row attaining it

HiGHS answers within its own 1e-7 of a problem it has scaled itself; the LP is therefore posed with the unit objective d / |d| and the value
is d.arg, which is what BAND in the tests is measured against.
"""
import numpy
from scipy.optimize import linprog

OPTIMAL, UNBOUNDED = 0, 3
LARGE = 1e6


def radius(rows):
    rows = numpy.asarray(rows, dtype=float)
    n = rows.shape[1] - 1
    c = numpy.append(numpy.zeros(n), -1.0)
    A = numpy.hstack([rows[:, 1:], numpy.ones((len(rows), 1))])
    res = linprog(c, A_ub=A, b_ub=rows[:, 0], bounds=[(None, None)] * (n + 1), method='highs')
    if res.status == 0:
        return False, -float(res.fun), numpy.asarray(res.x[:n], dtype=float)
    # unbounded (or "unbounded or infeasible", which cannot be infeasible: t is free below): bound t and keep the point
    res = linprog(c, A_ub=A, b_ub=rows[:, 0], bounds=[(-LARGE, LARGE)] * n + [(None, LARGE)], method='highs')
    if res.status != 0:
        raise RuntimeError(f'the radius LP ended with status {res.status}: {res.message}')
    r = -float(res.fun)
    return (True, numpy.inf, numpy.asarray(res.x[:n], dtype=float)) if r >= LARGE * (1 - 1e-9) else (False, r, numpy.asarray(res.x[:n], dtype=float))


def support(rows, d):
    rows, d = numpy.asarray(rows, dtype=float), numpy.asarray(d, dtype=float)
    n = rows.shape[1] - 1
    c = d / numpy.linalg.norm(d)
    res = linprog(-c, A_ub=rows[:, 1:], b_ub=rows[:, 0], bounds=[(None, None)] * n, method='highs')
    if res.status == 0:
        x = numpy.asarray(res.x, dtype=float)
        return OPTIMAL, float(d @ x), x
    if res.status == 3:
        return UNBOUNDED, numpy.inf, None
    # "unbounded or infeasible": in a box of half-width LARGE the optimum of an unbounded problem lies on the box
    res = linprog(-c, A_ub=rows[:, 1:], b_ub=rows[:, 0], bounds=[(-LARGE, LARGE)] * n, method='highs')
    if res.status != 0:
        raise RuntimeError(f'the support LP ended with status {res.status}: {res.message}')
    x = numpy.asarray(res.x, dtype=float)
    if numpy.max(numpy.abs(x)) >= LARGE * (1 - 1e-9):
        return UNBOUNDED, numpy.inf, None
    return OPTIMAL, float(d @ x), x


def erosion(p_rows, q_rows, E=None):
    p_rows = numpy.asarray(p_rows, dtype=float)
    out = p_rows.copy()
    for k, row in enumerate(p_rows):
        d = row[1:] if E is None else numpy.asarray(E, dtype=float).T @ row[1:]
        if not numpy.any(d != 0.0):
            continue
        st, h, _ = support(q_rows, d)
        if st == UNBOUNDED:
            return True, None
        out[k, 0] = row[0] - h
    return False, out


def containment(inner, outer):
    outer = numpy.asarray(outer, dtype=float)
    best, row, witness = -numpy.inf, -1, None
    for k, r in enumerate(outer):
        st, h, x = support(inner, r[1:])
        if st == UNBOUNDED:
            return numpy.inf, k, None
        if h - r[0] > best:
            best, row, witness = h - r[0], k, x
    return best, row, witness
