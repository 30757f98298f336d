"""An independent CPU statement of the transition graph of DESIGN §3.20 (numpy and scipy's HiGHS): the same definitions and thresholds
as ppopt_amd/transition.py, none of its code, and no box screen: every pair it is given gets its LP.

  pair_reference(rows_i, rows_j, Phi_i, phi_i, tol)  (status, radius, knife) of the ordered pair: T_ij = {theta in R_i : Phi_i theta +
                                                     phi_i in R_j}, rows unit [o | n]
  graph_reference(polys, Phi, phi, tol, pairs)       the same over a list of pairs (None: all R^2) -> {(i, j): (status, radius, knife)}
  steps_to_reference(n, edges, target)               (lower, upper) per region by enumerating every path

knife = True: the radius lies within KNIFE of tol, or a pulled-back row norm lies within a factor 10 of the ROW_EPS threshold; the device,
whose simplex rounds otherwise, may legitimately decide such a pair the other way.
"""
import numpy
from scipy.optimize import linprog

KNIFE = 1e-7
ROW_EPS = 1e-12
NO_EDGE, EDGE, UNBOUNDED = 'NO_EDGE', 'EDGE', 'UNBOUNDED'


def pulled_back(rows_j, Phi_i, phi_i, tol):
    """(unit rows [beta / s | a / s] of the rows of R_j that keep a normal, empty, knife)"""
    rows_j = numpy.asarray(rows_j, dtype=float)
    a = rows_j[:, 1:] @ Phi_i                      # row r: Phi_i^T n_r
    beta = rows_j[:, 0] - rows_j[:, 1:] @ phi_i
    s = numpy.sqrt(numpy.sum(a * a, axis=1))
    thr = ROW_EPS * max(1.0, float(numpy.max(numpy.abs(Phi_i))))
    keep = s > thr
    knife = bool(numpy.any((s >= thr / 10.0) & (s <= thr * 10.0)))
    empty = bool(numpy.any(~keep & (beta < -tol)))
    return numpy.column_stack([beta[keep] / s[keep], a[keep] / s[keep, None]]), empty, knife


def chebyshev(rows):
    """(unbounded, r, theta): the largest t with n.theta + t <= o over the unit rows, theta and t free"""
    n = rows.shape[1] - 1
    res = linprog(numpy.append(numpy.zeros(n), -1.0), A_ub=numpy.hstack([rows[:, 1:], numpy.ones((len(rows), 1))]), b_ub=rows[:, 0],
                  bounds=[(None, None)] * (n + 1), method='highs')
    if res.status == 0:
        return False, -float(res.fun), res.x[:n]
    if res.status == 3:
        return True, numpy.inf, None
    # "unbounded or infeasible" cannot be infeasible (t is free below): bound t and look at where the optimum lands
    res = linprog(numpy.append(numpy.zeros(n), -1.0), A_ub=numpy.hstack([rows[:, 1:], numpy.ones((len(rows), 1))]), b_ub=rows[:, 0],
                  bounds=[(None, None)] * n + [(None, 1e6)], method='highs')
    if res.status == 0 and -res.fun >= 1e6 * (1 - 1e-9):
        return True, numpy.inf, None
    if res.status == 0:
        return False, -float(res.fun), res.x[:n]
    raise RuntimeError(f'the radius LP ended with status {res.status}: {res.message}')


def pair_reference(rows_i, rows_j, Phi_i, phi_i, tol=1e-8):
    back, empty, knife = pulled_back(rows_j, numpy.asarray(Phi_i, dtype=float), numpy.asarray(phi_i, dtype=float), tol)
    if empty:
        return NO_EDGE, -numpy.inf, knife
    open_, r, _ = chebyshev(numpy.vstack([numpy.asarray(rows_i, dtype=float), back]))
    if open_:
        return UNBOUNDED, numpy.inf, knife
    return (EDGE if r > tol else NO_EDGE), r, knife or abs(r - tol) <= KNIFE


def graph_reference(polys, Phi, phi, tol=1e-8, pairs=None):
    R = len(polys)
    if pairs is None:
        pairs = [(i, j) for i in range(R) for j in range(R)]
    return {(int(i), int(j)): pair_reference(polys[i], polys[j], Phi[i], phi[i], tol) for i, j in pairs}


def steps_to_reference(n, edges, target):
    """(lower [n], upper [n]): over every path from a region that stops where it first enters the target, the fewest and the most
    edges; lower inf where no path arrives; upper inf where some path repeats a region or ends in a region without successor first"""
    succ = [[] for _ in range(n)]
    for i, j in edges:
        succ[int(i)].append(int(j))
    target = set(int(t) for t in target)
    lower, upper = numpy.full(n, numpy.inf), numpy.full(n, numpy.inf)
    for start in range(n):
        if start in target:
            lower[start] = upper[start] = 0.0
            continue
        lengths, endless = [], [False]

        def walk(node, path):
            if not succ[node]:
                endless[0] = True
            for nxt in succ[node]:
                if nxt in target:
                    lengths.append(len(path))
                elif nxt in path:
                    endless[0] = True
                else:
                    walk(nxt, path + [nxt])

        walk(start, [start])
        if lengths:
            lower[start] = min(lengths)
            upper[start] = numpy.inf if endless[0] else max(lengths)
    return lower, upper
