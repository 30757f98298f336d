"""Independent CPU references for the parameter-point kernels (k_qp_batch, the MIQP kernels, k_lp_batch): numpy, scipy and
mpmath only, no code of ppopt_amd.  A plain helper module (not a conftest), imported by tests/test_theta_reference_cpu.py and
tests/test_gpu_theta_kernels.py.

Programs are given at one parameter point: g = c + H theta, r = b + F theta, and

    min 1/2 x'Qx + g'x   s.t.  A x <= r,  the first n_eq rows equalities,  Q > 0.

* ``qp_certificate``: given a claimed active set, solve the equality-constrained KKT system of a maximal independent subset of
  the claimed rows (mpmath at 50 digits, or float64 with extended-precision iterative refinement for large systems) and accept
  it only if every row is primal feasible and every inequality multiplier is nonnegative, both to ``tol`` relative.  Q > 0
  makes such a point the unique optimum.
* ``qp_enumerate``: the answer with no input from the device, for n_c <= 12: every active set in float64, the first KKT point
  found, refined by ``qp_certificate``.
* ``feasibility_margin`` / ``feasibility_verdict``: max t s.t. A_I x + t ||A_i|| <= r_I, A_E x = r_E (HiGHS).
* ``lp_reference`` / ``milp_reference``: scipy's HiGHS LP and MILP with free continuous variables.
* ``miqp_brute_force``: every fixation substituted, each continuous QP by ``qp_enumerate``, the minimum objective.
"""
import itertools
from dataclasses import dataclass, field
from typing import List, Optional

import mpmath
import numpy
import scipy.optimize

DPS = 50
FEAS_EDGE = 1e-7          # |t| below this: knife-edge feasibility, never asserted either way
MP_MAX_DIM = 90           # KKT systems up to this size are solved in mpmath; larger ones in float64 + refinement


@dataclass
class QPCert:
    ok: bool
    x: numpy.ndarray
    lam: numpy.ndarray
    obj: float
    rows: List[int]                      # the independent rows the KKT system was solved on
    primal_margin: float                 # min over rows of (relative slack); >= -tol when ok
    dual_margin: float                   # min over inequality rows in ``rows`` of (relative multiplier); >= -tol when ok
    cond: float                          # condition number of the equilibrated KKT matrix
    reasons: List[str] = field(default_factory=list)


def independent_rows(A: numpy.ndarray, order: List[int], rtol: float = 1e-9) -> List[int]:
    """A maximal linearly independent subset of the rows ``order`` of A, greedily in that order (rows normalised)."""
    out: List[int] = []
    basis = numpy.zeros((0, A.shape[1]))
    for i in order:
        a = A[i]
        na = numpy.linalg.norm(a)
        if na == 0.0:
            continue
        v = a / na
        if len(basis):
            v = v - basis.T @ (basis @ v)
            v = v - basis.T @ (basis @ v)
        nv = numpy.linalg.norm(v)
        if nv > rtol:
            basis = numpy.vstack([basis, v / nv])
            out.append(i)
    return out


def _equilibrated_cond(K: numpy.ndarray) -> float:
    d = numpy.sqrt(numpy.max(numpy.abs(K), axis=1))
    d[d == 0] = 1.0
    return float(numpy.linalg.cond(K / d[:, None] / d[None, :]))


def _kkt_solve(Q, g, AS, rS, use_mp: bool):
    """[Q AS'; AS 0] [x; l] = [-g; rS]; returns (x, l) as float64 arrays (solved accurately)."""
    nx, k = Q.shape[0], AS.shape[0]
    K = numpy.block([[Q, AS.T], [AS, numpy.zeros((k, k))]])
    rhs = numpy.concatenate([-g, rS])
    if use_mp:
        with mpmath.workdps(DPS):
            sol = mpmath.lu_solve(mpmath.matrix(K.tolist()), mpmath.matrix(rhs.tolist()))
            v = numpy.array([float(sol[i]) for i in range(nx + k)])
    else:
        Kl, rl = K.astype(numpy.longdouble), rhs.astype(numpy.longdouble)
        v = numpy.linalg.solve(K, rhs)
        for _ in range(4):
            res = (rl - Kl @ v.astype(numpy.longdouble)).astype(numpy.float64)
            v = v + numpy.linalg.solve(K, res)
    return v[:nx], v[nx:]


def qp_certificate(Q, g, A, r, n_eq: int, active, order_hint=None, tol: float = 1e-12, use_mp: Optional[bool] = None) -> QPCert:
    """Certificate form: the KKT point of the claimed active set (equality rows always included) and its margins.  Rows are
    taken into the independent subset equality rows first, then the claimed inequality rows in the order of ``order_hint``
    (e.g. decreasing claimed multipliers), so that weakly active rows are the ones dropped."""
    Q, g, A, r = (numpy.asarray(v, dtype=numpy.float64) for v in (Q, g, A, r))
    nc, nx = A.shape
    active = numpy.asarray(active, dtype=bool).reshape(nc)
    claimed = [i for i in range(n_eq, nc) if active[i]]
    if order_hint is not None:
        claimed.sort(key=lambda i: -float(order_hint[i]))
    rows = independent_rows(A, list(range(n_eq)) + claimed)
    AS, rS = A[rows].reshape(-1, nx), r[rows]
    if use_mp is None:
        use_mp = nx + len(rows) <= MP_MAX_DIM
    K = numpy.block([[Q, AS.T], [AS, numpy.zeros((len(rows), len(rows)))]])
    cond = _equilibrated_cond(K)
    x, l = _kkt_solve(Q, g, AS, rS, use_mp)
    lam = numpy.zeros(nc)
    lam[rows] = l
    # margins in extended precision
    xl = x.astype(numpy.longdouble)
    Al = A.astype(numpy.longdouble)
    s = (r.astype(numpy.longdouble) - Al @ xl).astype(numpy.float64)
    sc = numpy.abs(r) + (numpy.abs(A) @ numpy.abs(x)) + 1e-300
    rel_s = s / sc
    reasons = []
    pm = numpy.concatenate([rel_s[n_eq:], -numpy.abs(rel_s[:n_eq])]) if nc else numpy.zeros(0)
    primal_margin = float(pm.min()) if pm.size else numpy.inf
    if primal_margin < -tol:
        reasons.append(f'primal infeasible by {-primal_margin:.3g} relative')
    grad = numpy.abs(Q @ x) + numpy.abs(g)
    lsc = (numpy.max(grad) if grad.size else 0.0) / numpy.maximum(numpy.max(numpy.abs(A), axis=1), 1e-300) + 1e-300
    ineq_rows = [i for i in rows if i >= n_eq]
    dual_margin = float(min((lam[i] / lsc[i] for i in ineq_rows), default=numpy.inf))
    if dual_margin < -tol:
        reasons.append(f'negative multiplier by {-dual_margin:.3g} relative')
    obj = float(0.5 * xl @ (Q.astype(numpy.longdouble) @ xl) + g.astype(numpy.longdouble) @ xl)
    return QPCert(not reasons, x, lam, obj, rows, primal_margin, dual_margin, cond, reasons)


def qp_enumerate(Q, g, A, r, n_eq: int, tol: float = 1e-9) -> Optional[QPCert]:
    """The optimum with no device input (n_c <= 12): every active set of the inequality rows in float64, smallest first; the first
    KKT point that is primal and dual feasible to ``tol`` is refined in mpmath.  None: no KKT point (infeasible)."""
    Q, g, A, r = (numpy.asarray(v, dtype=numpy.float64) for v in (Q, g, A, r))
    nc, nx = A.shape
    assert nc <= 12
    eq = independent_rows(A, list(range(n_eq)))
    ineq = list(range(n_eq, nc))
    for k in range(0, min(nx - len(eq), len(ineq)) + 1):
        for S in itertools.combinations(ineq, k):
            rows = eq + list(S)
            if len(independent_rows(A, rows)) < len(rows):
                continue
            AS = A[rows].reshape(-1, nx)
            K = numpy.block([[Q, AS.T], [AS, numpy.zeros((len(rows), len(rows)))]])
            try:
                v = numpy.linalg.solve(K, numpy.concatenate([-g, r[rows]]))
            except numpy.linalg.LinAlgError:
                continue
            x, l = v[:nx], v[nx:]
            sc = numpy.abs(r) + numpy.abs(A) @ numpy.abs(x) + 1e-300
            s = (r - A @ x) / sc
            if nc and (numpy.any(s[n_eq:] < -tol) or numpy.any(numpy.abs(s[:n_eq]) > tol)):
                continue
            if numpy.any(l[len(eq):] < -tol * (1 + numpy.max(numpy.abs(l), initial=0.0))):
                continue
            act = numpy.zeros(nc, dtype=bool)
            act[list(S)] = True
            cert = qp_certificate(Q, g, A, r, n_eq, act, tol=1e-10, use_mp=True)
            if cert.ok:
                return cert
    return None


def feasibility_margin(A, r, n_eq: int) -> float:
    """max t s.t. A_i x + t ||A_i|| <= r_i (inequalities), A_e x = r_e, t <= 1 (HiGHS); -inf when even that is infeasible."""
    A, r = numpy.asarray(A, dtype=numpy.float64), numpy.asarray(r, dtype=numpy.float64)
    nc, nx = A.shape
    nrm = numpy.linalg.norm(A, axis=1)
    zero = nrm == 0
    if numpy.any(zero[n_eq:] & (r[n_eq:] < 0)) or numpy.any(zero[:n_eq] & (r[:n_eq] != 0)):
        return -numpy.inf
    nrm[zero] = 1.0
    I = [i for i in range(n_eq, nc) if not zero[i]]
    E = [i for i in range(n_eq) if not zero[i]]
    cost = numpy.zeros(nx + 1)
    cost[-1] = -1.0
    A_ub = numpy.hstack([A[I] / nrm[I, None], numpy.ones((len(I), 1))]) if I else None
    b_ub = r[I] / nrm[I] if I else None
    A_eq = numpy.hstack([A[E] / nrm[E, None], numpy.zeros((len(E), 1))]) if E else None
    b_eq = r[E] / nrm[E] if E else None
    res = scipy.optimize.linprog(cost, A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=b_eq, bounds=[(None, None)] * nx + [(None, 1.0)],
                                 method='highs')
    if res.status == 2:
        return -numpy.inf
    assert res.status == 0, res.message
    return float(res.x[-1])


def feasibility_verdict(A, r, n_eq: int) -> str:
    """'feasible', 'infeasible' or 'edge' (|t| <= FEAS_EDGE: counted, never asserted)."""
    t = feasibility_margin(A, r, n_eq)
    return 'feasible' if t > FEAS_EDGE else ('infeasible' if t < -FEAS_EDGE else 'edge')


def lp_reference(A, b, c, eq):
    """min c'x s.t. A x <= b (rows with eq[i] equalities), x free.  (status 0 optimal / 1 infeasible / 2 unbounded, objective)."""
    A, b = numpy.asarray(A, dtype=numpy.float64), numpy.asarray(b, dtype=numpy.float64)
    eq = numpy.asarray(eq, dtype=bool)
    c = numpy.zeros(A.shape[1]) if c is None else numpy.asarray(c, dtype=numpy.float64)
    I, E = ~eq, eq
    res = scipy.optimize.linprog(c, A_ub=A[I] if I.any() else None, b_ub=b[I] if I.any() else None, A_eq=A[E] if E.any() else None,
                                 b_eq=b[E] if E.any() else None, bounds=[(None, None)] * A.shape[1], method='highs')
    st = {0: 0, 2: 1, 3: 2}[res.status]
    return st, (float(res.fun) if st == 0 else None)


def milp_reference(A, b, c, eq, binary_indices):
    """min c'x s.t. A x <= b (eq rows equalities), x_j in {0, 1} for j in binary_indices, the rest free (HiGHS MILP)."""
    A, b, c = (numpy.asarray(v, dtype=numpy.float64) for v in (A, b, c))
    eq = numpy.asarray(eq, dtype=bool)
    n = A.shape[1]
    lb, ub = numpy.full(n, -numpy.inf), numpy.full(n, numpy.inf)
    integrality = numpy.zeros(n)
    lb[binary_indices], ub[binary_indices], integrality[binary_indices] = 0, 1, 1
    lo = numpy.where(eq, b, -numpy.inf)
    res = scipy.optimize.milp(c, constraints=scipy.optimize.LinearConstraint(A, lo, b), integrality=integrality,
                              bounds=scipy.optimize.Bounds(lb, ub))
    if res.status == 2:
        return 1, None
    assert res.status == 0, res.message
    return 0, float(res.fun)


def miqp_brute_force(Q, c, H, A, b, F, n_eq: int, binary_indices, fixations, theta, check_tol: float = 1e-9):
    """The MIQP at theta over the given fixations (rows [n_x] binaries' values): per fixation the continuous QP by qp_enumerate
    (rows without continuous content are checked on their own), objective 1/2 x'Qx + (c + H theta)'x of the full x.
    Returns (best objective or None, per-fixation objectives (None: infeasible))."""
    Q, c, H, A, b, F = (numpy.asarray(v, dtype=numpy.float64) for v in (Q, c, H, A, b, F))
    theta = numpy.asarray(theta, dtype=numpy.float64).reshape(-1)
    nx = A.shape[1]
    bi = list(binary_indices)
    ci = [j for j in range(nx) if j not in bi]
    g_full = c.reshape(-1) + H @ theta
    r_full = b.reshape(-1) + F @ theta
    Qs = 0.5 * (Q + Q.T)
    objs = []
    for y in numpy.asarray(fixations, dtype=numpy.float64).reshape(-1, len(bi)):
        r = r_full - A[:, bi] @ y
        Ac = A[:, ci]
        cont = numpy.any(Ac != 0, axis=1)
        ok = True
        for i in numpy.flatnonzero(~cont):
            if (i < n_eq and abs(r[i]) > check_tol) or (i >= n_eq and r[i] < -check_tol):
                ok = False
        if not ok:
            objs.append(None)
            continue
        keep = numpy.flatnonzero(cont)
        ne = int(numpy.sum(keep < n_eq))
        g = g_full[ci] + Qs[numpy.ix_(ci, bi)] @ y
        cert = qp_enumerate(Qs[numpy.ix_(ci, ci)], g, Ac[keep], r[keep], ne)
        if cert is None:
            objs.append(None)
            continue
        objs.append(cert.obj + float(g_full[bi] @ y + 0.5 * y @ Qs[numpy.ix_(bi, bi)] @ y))
    feas = [o for o in objs if o is not None]
    return (min(feas) if feas else None), objs


def compare_qp(cert: QPCert, Q, g, A, x, lam, tol: float):
    """Normwise relative errors of a device answer (x, lam) against a certificate: dict of x / lam / obj errors."""
    x, lam = numpy.asarray(x, dtype=numpy.float64), numpy.asarray(lam, dtype=numpy.float64)
    x_unc = numpy.linalg.solve(Q, -numpy.asarray(g, dtype=numpy.float64))
    xs = max(numpy.max(numpy.abs(cert.x), initial=0.0), numpy.max(numpy.abs(x_unc), initial=0.0), 1e-300)
    gs = numpy.max(numpy.abs(g), initial=0.0) / max(numpy.max(numpy.abs(A), initial=0.0), 1e-300)
    ls = max(numpy.max(numpy.abs(cert.lam), initial=0.0), gs, 1e-300)
    xl = x.astype(numpy.longdouble)
    obj = float(0.5 * xl @ (numpy.asarray(Q, dtype=numpy.longdouble) @ xl) + numpy.asarray(g, dtype=numpy.longdouble) @ xl)
    osc = max(abs(cert.obj), float(0.5 * numpy.abs(cert.x) @ numpy.abs(Q) @ numpy.abs(cert.x) + numpy.abs(g) @ numpy.abs(cert.x)), 1e-300)
    return {'x': float(numpy.max(numpy.abs(x - cert.x), initial=0.0) / xs),
            'lam': float(numpy.max(numpy.abs(lam - cert.lam), initial=0.0) / ls),
            'obj': abs(obj - cert.obj) / osc, 'tol': tol}


def qp_tolerance(cert: QPCert) -> float:
    return max(1e-9, 4e-16 * cert.cond)
