"""MPMIQP_Program: a multiparametric QP some of whose variables are binary (reference: mpmiqp_program.py:11-148).

    min_{x,y}  1/2 [x,y]' Q [x,y] + theta' H' [x,y] + c' [x,y] + c_c + c_t' theta + 1/2 theta' Q_t theta

Feasibility questions do not involve the objective, so presolve and the binary tree are those of MPMILP_Program
(device-batched LPs); only the substitution of a fixation carries the quadratic terms.
"""
from typing import List, Optional, Union

import numpy

from .mpmilp_program import MPMILP_Program
from .mpqp_program import MPQP_Program
from .solver import Solver, SolverOutput


class MPMIQP_Program(MPMILP_Program):
    def __init__(self, A, b, c, H, Q, A_t, b_t, F, binary_indices: List, c_c=None, c_t=None, Q_t=None,
                 equality_indices=None, solver: Optional[Solver] = None, post_process: bool = True):
        self.Q = numpy.asarray(Q, dtype=numpy.float64)
        super().__init__(A, b, c, H, A_t, b_t, F, binary_indices, c_c, c_t, Q_t, equality_indices, solver,
                         post_process=False)
        if post_process:
            self.post_process()

    def evaluate_objective(self, x: numpy.ndarray, theta_point: numpy.ndarray) -> float:
        v = 0.5 * x.T @ self.Q @ x + theta_point.T @ self.H.T @ x + self.c.T @ x + self.c_c \
            + self.c_t.T @ theta_point + 0.5 * theta_point.T @ self.Q_t @ theta_point
        return float(v[0, 0])

    def generate_substituted_problem(self, fixed_combination: Union[numpy.ndarray, List[int]], deferred: bool = False):
        """The continuous mpQP with the binaries fixed (mpmiqp_program.py:70-115): the binary block of Q moves into
        the constant, the mixed block into the linear term.  ``deferred`` (the enumeration's batch construction): the presolve's
        redundancy LPs are left to the caller (``_redundancy_request`` / ``_redundancy_apply``) and the diagnostic LPs are not posed."""
        A_cont, b, F, eq, y = self._substituted_rows(fixed_combination)
        ci, bi = self.cont_indices, self.binary_indices
        Q_c = self.Q[:, ci][ci]
        Q_d = self.Q[:, bi][bi]
        Q_mix = self.Q[:, ci][bi]
        c = self.c[ci] + Q_mix.T @ y
        c_c = self.c_c + self.c[bi].T @ y + 0.5 * y.T @ Q_d @ y
        H_c = self.H[ci]
        H_d = self.H[bi]
        c_t = self.c_t + (y.T @ H_d).T
        return MPQP_Program(A_cont, b, c, H_c, Q_c, self.A_t, self.b_t, F, c_c, c_t, self.Q_t, eq, self.solver,
                            post_process=not deferred, _diagnostics=not deferred)

    def generate_relaxed_problem(self, process: bool = True) -> MPQP_Program:
        A, b, F = self._relaxation_rows()
        return MPQP_Program(A, b, self.c, self.H, self.Q, self.A_t, self.b_t, F, self.c_c, self.c_t, self.Q_t,
                            self.equality_indices, self.solver, post_process=process)

    # ---- the MIQP at fixed parameter points (device: mpc_miqp_solve_batch, csrc/qp.hpp) ---------------------------------------
    def theta_blocks(self) -> dict:
        """The fixation-independent arrays of the MIQP at a parameter point, in z = [1; theta; y] (include/mpcombi.h,
        mpc_miqp_solve_batch).  Every row of A is one of three kinds:

        * LCP rows carry continuous content: with x_c = X0 z - Gt' lambda the slacks are s = UV z + W lambda, W = A_c Q_c^-1 A_c'.
          Equality rows that are linearly dependent in A_c (they differ only in their binary columns) keep an independent subset;
          the residual of each dependent row against it is affine in z and becomes a check row.
        * check rows have theta content but no continuous content: their sign is decided on z alone.
        * pure-binary rows have neither; leaf_feasibility() already removed every fixation that violates them.

        The objective is 1/2 x_c' Q_c x_c + (G z)' x_c + 1/2 z' K z, constants included.  Cached per program, keyed like
        ``_substituted_rows``.  Raises NotImplementedError when Q_c is not positive definite."""
        key = (id(self.A), id(self.b), id(self.F), id(self.Q), self.A.shape, tuple(self.equality_indices))
        cache = getattr(self, '_theta_blocks', None)
        if cache is not None and cache[0] == key:
            return cache[1]
        ci, bi = list(self.cont_indices), list(self.binary_indices)
        nt, nb, nxc = self.num_t(), len(bi), len(ci)
        Qs = 0.5 * (self.Q + self.Q.T)
        Q_c = Qs[numpy.ix_(ci, ci)]
        try:
            L = numpy.linalg.cholesky(Q_c)
        except numpy.linalg.LinAlgError:
            L = None
        if L is None or numpy.min(numpy.abs(numpy.diag(L))) ** 2 < 1e-12 * max(1.0, float(numpy.max(numpy.abs(Q_c)))):
            raise NotImplementedError('the MIQP at a parameter point needs a positive definite continuous Hessian Q_c '
                                      '(a positive semidefinite Q_c is outside the device QP, as for MPQP_Program.solve_theta_batch)')
        A_c, A_b = self.A[:, ci], self.A[:, bi]
        # right-hand side of every row in z: s = R z - A_c x_c
        R = numpy.hstack([self.b.reshape(-1, 1), self.F, -A_b])
        cont = [not numpy.allclose(A_c[i], 0 * A_c[i]) for i in range(self.num_constraints())]
        par = [not numpy.allclose(self.F[i], 0 * self.F[i]) for i in range(self.num_constraints())]
        eq_set = set(self.equality_indices)
        eq_rows = [i for i in self.equality_indices if cont[i]]
        indep, dep = [], []
        for i in eq_rows:
            if numpy.linalg.matrix_rank(A_c[indep + [i]]) > len(indep):
                indep.append(i)
            else:
                dep.append(i)
        ineq_rows = [i for i in range(self.num_constraints()) if i not in eq_set and cont[i]]
        lcp = indep + ineq_rows
        check, check_eq = [], []
        for i in range(self.num_constraints()):
            if not cont[i] and par[i]:
                check.append(R[i])
                check_eq.append(i in eq_set)
        if dep:
            # A_c[d] = alpha' A_c[indep]: with the independent rows holding, the slack of row d is (R_d - alpha' R_indep) z
            alpha = numpy.linalg.lstsq(A_c[indep].T, A_c[dep].T, rcond=None)[0]
            for j, d in enumerate(dep):
                check.append(R[d] - alpha[:, j] @ R[indep])
                check_eq.append(True)
        nz = 1 + nt + nb
        G = numpy.hstack([self.c[ci].reshape(-1, 1), self.H[ci], Qs[numpy.ix_(ci, bi)]])
        A_l = A_c[lcp]
        QiA = numpy.linalg.solve(Q_c, A_l.T)                     # Q_c^-1 A_l'
        QiG = numpy.linalg.solve(Q_c, G)
        K = numpy.zeros((nz, nz))
        t, y = slice(1, 1 + nt), slice(1 + nt, nz)
        K[0, 0] = 2.0 * float(numpy.asarray(self.c_c).reshape(-1)[0])
        K[0, t] = K[t, 0] = numpy.asarray(self.c_t).reshape(-1)
        K[0, y] = K[y, 0] = self.c[bi].reshape(-1)
        K[t, t] = 0.5 * (self.Q_t + self.Q_t.T)
        K[y, y] = Qs[numpy.ix_(bi, bi)]
        K[t, y] = self.H[bi].T
        K[y, t] = self.H[bi]
        blocks = {'n_c': len(lcp), 'n_eq': len(indep), 'n_x': self.num_x(), 'n_t': nt, 'n_b': nb, 'n_rows': self.num_constraints(),
                  'W': A_l @ QiA, 'UV': R[lcp] + A_l @ QiG, 'X0': -QiG, 'Gt': QiA.T, 'Q_c': Q_c, 'G': G, 'K': K,
                  'check': numpy.array(check, dtype=numpy.float64).reshape(-1, nz), 'check_eq': numpy.array(check_eq, dtype=numpy.uint8),
                  'binary_index': numpy.array(bi, dtype=numpy.int32), 'lcp_row': numpy.array(lcp, dtype=numpy.int32),
                  'lcp_rows': lcp, 'dependent_rows': dep}
        self._theta_blocks = (key, blocks, (self.A, self.b, self.F, self.Q))      # (the arrays are held: their ids stay theirs)
        return blocks

    def solve_theta(self, theta_point: numpy.ndarray) -> Optional[SolverOutput]:
        """The MIQP at a fixed theta (mpmiqp_program.py:55-69): the minimum over the feasible fixations of their QPs, the first
        fixation on ties.  ``obj`` includes the constant terms, ``sol`` is the full [x, y] vector, ``slack`` covers every row,
        ``active_set`` is the rows with |slack| <= 1e-10 and ``dual`` the winning fixation's multipliers over all rows.  Like
        MPMILP_Program.solve_theta and the reference, theta is not checked against A_t theta <= b_t.  None when no fixation
        has a solution.  Equal, bit for bit, to ``solve_theta_batch`` of the one point."""
        return self.solve_theta_batch(numpy.asarray(theta_point, dtype=numpy.float64).reshape(1, -1))[0]

    def solve_theta_batch(self, theta_points: numpy.ndarray, leaves: Optional[List[List[int]]] = None) -> List[Optional[SolverOutput]]:
        """``solve_theta`` for many parameter points (theta_points [m, n_theta]): every (point, feasible fixation) pair as one LCP
        on the device, one call per chunk of points whose 12 bytes per pair stay within Solver.MILP_BATCH_BYTES.  ``leaves``:
        the fixations to consider (default: feasible_combinations()).  Raises MpcError when a point's minimum is uncertain (a pair at
        the iteration limit) instead of reporting it as None."""
        from . import _lib
        th = numpy.ascontiguousarray(theta_points, dtype=numpy.float64).reshape(-1, self.num_t())
        B = self.theta_blocks()
        Y = numpy.asarray(self.feasible_combinations() if leaves is None else leaves, dtype=numpy.float64).reshape(-1, len(self.binary_indices))
        out: List[Optional[SolverOutput]] = [None] * len(th)
        if len(Y) == 0 or len(th) == 0:
            return out
        step = max(1, int(self.solver.MILP_BATCH_BYTES // (12 * len(Y))))
        for lo in range(0, len(th), step):
            hi = min(len(th), lo + step)
            status, _, obj, x, lam, _ = _lib.miqp_solve_batch(B, Y, th[lo:hi], device=self.solver.device)
            if numpy.any(status == 3):
                raise _lib.MpcError(f'the MIQP at {int(numpy.sum(status == 3))} parameter points has a fixation whose QP stopped at the '
                                    f'iteration limit (first: point {lo + int(numpy.flatnonzero(status == 3)[0])}): its minimum is unknown')
            for j in numpy.flatnonzero(status == 0):
                tp, xp = th[lo + j].reshape(-1, 1), x[j].reshape(-1, 1)
                slack = (self.b + self.F @ tp - self.A @ xp).ravel()
                out[lo + j] = SolverOutput(float(obj[j]), x[j].copy(), slack, numpy.flatnonzero(numpy.abs(slack) <= 1e-10), lam[j].copy())
        return out
