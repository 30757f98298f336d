// qp.hpp -- the strictly convex QP of an mpQP at fixed parameter points, batched: one wavefront per point (gfx950).
//
// Reference: MPQP_Program.solve_theta (mpqp_program.py:109-143) -> Solver.solve_qp -> quadprog / gurobi / daqp
// (solver_interface/quad_prog_interface.py:16-89), one QP per call.  Callers: sample_theta_space (mplp_program.py:632-664,
// the seeds of the graph algorithms), Solution.verify_theta / verify_solution (solution.py:114-174).
//
//     min 1/2 x'Qx + (c + H theta)'x   s.t.  A x <= b + F theta  (first n_eq rows equalities),   Q > 0
//
// With x = -Q^-1 (c + H theta + A' lambda) the KKT conditions are a linear complementarity problem in the multipliers alone,
//     s = q(theta) + W lambda,   s >= 0, lambda >= 0, s'lambda = 0      (s_e = 0, lambda_e free on equality rows)
// with W = A Q^-1 A' and q = UV [1; theta] -- the blocks the combinatorial kernels already keep on the device (mpc_create).
// The LCP is solved by Lemke's complementary pivoting on an LDS dictionary (lp_engine.hpp's pivot): the multipliers of the
// equality rows enter first and their slacks are deleted (a principal block pivot), the covering variable z0 enters on the
// most negative q_i, then the complement of whatever left enters until z0 leaves (solved) or no row limits the entering
// variable (ray termination: the QP is infeasible at this theta).  W is positive semidefinite, so Lemke terminates in one
// of the two.  Ratio ties (to QP_TOL_TIE) go to z0's row, then lexicographically (qp_lex_row), then to the lowest variable id.
// The LCP is solved in the symmetric diagonal scaling s' = D s, lambda = D lambda', D = diag(W_ii)^-1/2 (1 on a zero row):
// D W D keeps W's semidefiniteness and complementarity and has a unit diagonal, so the absolute pivot tolerances (TOL_PIV,
// the equality pivot, the start test) are relative to the rows' own scale.  Without it a Q of 1e10 I with unit rows left
// every entry of W below TOL_PIV and feasible points ended in ray termination.  The multipliers are mapped back at the end.
// An equality row that depends on the equality rows before it (its pivot entry vanishes) is dropped when it is consistent at
// this theta (lambda_e = 0) and makes the point infeasible when it is not.
#pragma once
#include "lp_engine.hpp"
#include "../../include/mpcombi.h"

namespace mpc {

enum : int { QP_OPTIMAL = 0, QP_INFEASIBLE = 1, QP_ITERLIMIT = 3 };
constexpr double QP_TOL_DEP = 1e-10;   // scaled pivot entry below which an equality row counts as dependent on the earlier ones
constexpr double QP_TOL_TIE = 1e-12;   // ratio-test rows whose scaled right-hand sides differ by less tie (qp_lex_row)

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}

// ---- the LCP of one point: dictionary, complementary pivoting, multipliers (shared by k_qp_batch and the MIQP kernels) ----
// Dictionary of the scaled LCP: s'_i = d_i q_i - sum_j (-d_i W_ij d_j) lambda'_j - (-1) z0 with q_i = qf(i), d_i = W_ii^-1/2;
// the cost row (index nc) is unused.  d is left in dv[nc] (LDS) for qp_multipliers.
template <class QF>
__device__ inline void qp_lcp_dict(Lp &lp, int nc, int n_eq, const double *__restrict__ W, double *dv, QF qf) {
    const int lane = lane_id(), ld = lp.ld, ID_Z0 = 2 * nc;
    double *T = lp.T;
    lp.m = nc; lp.n = 0; lp.na = nc + 1; lp.iters = 0; lp.max_iter = 50 * nc + 100; lp.growth = 0.0;
    wave_sync();
    for (int i = lane; i < nc; i += 64) { const double w = W[(size_t)i * nc + i]; dv[i] = w > 0.0 ? 1.0 / sqrt(w) : 1.0; }
    wave_sync();
    for (int i = lane; i <= nc; i += 64) {
        double *Ti = T + (size_t)i * ld;
        double q = 0.0;
        const double di = i < nc ? dv[i] : 0.0;
        if (i < nc) q = di * qf(i);
        Ti[0] = q;
        for (int j = 0; j < nc; ++j) Ti[1 + j] = i < nc ? -(W[(size_t)i * nc + j] * (di * dv[j])) : 0.0;
        Ti[nc + 1] = (i >= n_eq && i < nc) ? -1.0 : 0.0;
        if (i < nc) { lp.rowvar[i] = nc + i; lp.rowkind[i] = i < n_eq ? RK_EQ : RK_INEQ; }
    }
    for (int j = lane; j <= nc + 1; j += 64) lp.colvar[j] = j == 0 ? -1 : (j <= nc ? j - 1 : ID_Z0);
    wave_sync();
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The leaving row of a degenerate step, lexicographically.  The rows whose ratio is within QP_TOL_TIE (in the units of the
// scaled right-hand side) of the minimum rmin all tie; z0's row wins among them, otherwise the rows are ranked by the rows of
// B^-1 divided by their pivot entries, taken in the order of the initial basic variables s_k (column k of B^-1 is the
// dictionary column of s_k while s_k is nonbasic, the unit vector of its row while it is basic), until one row is left; then
// the lowest variable id.  Without it a run of degenerate pivots can reach an almost-complementary basis whose entering column
// is zero (a secondary ray): a feasible point reported infeasible.  br (the plain rule's row) is returned when nothing ties.
// Equality slacks (k < n_eq) were deleted with their columns and take no part.  Rows per lane: i = lane + 64 s, s < 32.
__device__ inline int qp_lex_row(const Lp &lp, int nc, int n_eq, int q, double rmin, int br) {
    const int lane = lane_id(), ld = lp.ld, ID_Z0 = 2 * nc;
    const double *T = lp.T;
    unsigned tie = 0;
    int ntie = 0, z0 = -1;
    for (int i = lane, b = 0; i < nc; i += 64, ++b) {
        if (lp.rowkind[i] != RK_INEQ) continue;
        const double a = T[(size_t)i * ld + q];
        if (!(a > TOL_PIV) || !(fmax(T[(size_t)i * ld], 0.0) <= rmin * a + QP_TOL_TIE)) continue;
        tie |= 1u << b;
        ++ntie;
        if (lp.rowvar[i] == ID_Z0) z0 = i;
    }
    z0 = wave_max_i(z0);
    if (z0 >= 0) return z0;
    ntie = wave_sum_i(ntie);
    if (ntie <= 1) return br;
    for (int k = n_eq; k < nc && ntie > 1; ++k) {
        int jc = -1, rb = -1;
        for (int j = 1 + lane; j <= lp.na; j += 64) if (lp.colvar[j] == nc + k) jc = j;
        jc = wave_max_i(jc);
        if (jc < 0) {
            for (int i = lane; i < nc; i += 64) if (lp.rowvar[i] == nc + k) rb = i;
            rb = wave_max_i(rb);
        }
        double vmin = INFINITY;
        for (int i = lane, b = 0; i < nc; i += 64, ++b)
            if (tie >> b & 1u) {
                const double v = jc >= 0 ? T[(size_t)i * ld + jc] : (i == rb ? 1.0 : 0.0);
                vmin = fmin(vmin, v / T[(size_t)i * ld + q]);
            }
        vmin = wave_min(vmin);
        ntie = 0;
        for (int i = lane, b = 0; i < nc; i += 64, ++b)
            if (tie >> b & 1u) {
                const double v = jc >= 0 ? T[(size_t)i * ld + jc] : (i == rb ? 1.0 : 0.0);
                if (v <= vmin * T[(size_t)i * ld + q] + QP_TOL_TIE) ++ntie;
                else tie &= ~(1u << b);
            }
        ntie = wave_sum_i(ntie);
    }
    // the lowest variable id among the rows left
    int bv = 0x7fffffff, bi = -1;
    for (int i = lane, b = 0; i < nc; i += 64, ++b)
        if ((tie >> b & 1u) && lp.rowvar[i] < bv) { bv = lp.rowvar[i]; bi = i; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int ov = __shfl_xor(bv, off), oi = __shfl_xor(bi, off);
        if (ov < bv) { bv = ov; bi = oi; }
    }
    return bi >= 0 ? bi : br;
}

// Lemke's method on the dictionary of qp_lcp_dict: QP_OPTIMAL, QP_INFEASIBLE or QP_ITERLIMIT (wave-uniform)
__device__ inline int qp_lemke(Lp &lp, int nc, int n_eq) {
    const int lane = lane_id(), ld = lp.ld, ID_Z0 = 2 * nc, ID_RETIRED = 2 * nc + 1;   // a retired row is neither slack nor multiplier
    double *T = lp.T;
    int st = QP_OPTIMAL;
    // equality rows: lambda_e enters on its own row (largest remaining diagonal first would be safer; the scaled W_ee is 1
    // for independent equality rows), the slack s_e is fixed at zero and its column deleted
    for (int e = 0; e < n_eq && st == QP_OPTIMAL; ++e) {
        int q = -1;
        for (int j = 1 + lane; j <= lp.na; j += 64) if (lp.colvar[j] == e) q = j;
        q = wave_max_i(q);
        if (q < 0) { st = QP_INFEASIBLE; break; }
        const double *Te = T + (size_t)e * ld;
        if (!(fabs(Te[q]) > QP_TOL_DEP)) {
            // row e is a combination of the equality rows pivoted before it: its multiplier entries vanish with T_ee and T_e0 is the
            // residual of the dependence at this theta.  Consistent: lambda_e = 0 and the row is retired; otherwise infeasible.
            double big = 0.0;
            for (int j = 1 + lane; j <= lp.na; j += 64) big = fmax(big, fabs(Te[j]));
            big = wave_max(big);
            if (big > QP_TOL_DEP || !(fabs(Te[0]) <= QP_TOL_DEP)) { st = QP_INFEASIBLE; break; }
            lp_drop_col(lp, q);
            if (lane == 0) { lp.rowkind[e] = RK_DEAD; lp.rowvar[e] = ID_RETIRED; }
            wave_sync();
            continue;
        }
        lp_pivot(lp, e, q);
        lp_drop_col(lp, q);
        if (lane == 0) lp.rowkind[e] = RK_FREE;
        wave_sync();
    }
    if (st == QP_OPTIMAL) {
        // most negative value among the inequality rows
        double vmin = 0.0; int key = 0, r = -1;
        for (int i = lane; i < nc; i += 64)
            if (lp.rowkind[i] == RK_INEQ) { const double v = T[(size_t)i * ld]; if (r < 0 || v < vmin) { vmin = v; r = i; } }
        reduce_min_first(vmin, key, r);
        if (r >= 0 && vmin < -1e-12) {
            int qz = -1;
            for (int j = 1 + lane; j <= lp.na; j += 64) if (lp.colvar[j] == ID_Z0) qz = j;
            qz = wave_max_i(qz);
            int left = lp.rowvar[r];
            lp_pivot(lp, r, qz);
            for (;;) {
                if (lp.iters > lp.max_iter) { st = QP_ITERLIMIT; break; }
                const int enter = left < nc ? left + nc : left - nc;   // the complement of the variable that left
                int q = -1;
                for (int j = 1 + lane; j <= lp.na; j += 64) if (lp.colvar[j] == enter) q = j;
                q = wave_max_i(q);
                if (q < 0) { st = QP_INFEASIBLE; break; }           // its column was deleted: cannot happen for inequality rows
                // ratio test over the sign-restricted rows (the free multipliers of the equality rows never leave)
                double best = INFINITY; int bz = 0, bvar = 0, br = -1;
                for (int i = lane; i < nc; i += 64) {
                    if (lp.rowkind[i] != RK_INEQ) continue;
                    const double a = T[(size_t)i * ld + q];
                    if (!(a > TOL_PIV)) continue;
                    const double ratio = fmax(T[(size_t)i * ld], 0.0) / a;
                    const int isz = lp.rowvar[i] == ID_Z0 ? 1 : 0, var = lp.rowvar[i];
                    if (bland_better(ratio, isz, var, best, bz, bvar, br)) { best = ratio; bz = isz; bvar = var; br = i; }
                }
                double piv = 0.0;
                reduce_ratio(best, piv, bz, bvar, br, true);
                if (br < 0) { st = QP_INFEASIBLE; break; }          // ray termination
                br = qp_lex_row(lp, nc, n_eq, q, best, br);
                left = lp.rowvar[br];
                lp_pivot(lp, br, q);
                if (left == ID_Z0) break;                             // z0 left the basis: complementary solution
            }
        }
    }
    return st;
}

// the multipliers of the final dictionary into lamv[nc] (zero unless optimal); lamv holds the scaling d of qp_lcp_dict on entry:
// lambda_v = d_v lambda'_v is formed in column 0 of the final tableau (not read again) before lamv is overwritten
__device__ inline void qp_multipliers(const Lp &lp, int nc, int st, double *lamv) {
    const int lane = lane_id();
    if (st == QP_OPTIMAL)
        for (int i = lane; i < nc; i += 64) { const int v = lp.rowvar[i]; if (v < nc) lp.T[(size_t)i * lp.ld] *= lamv[v]; }
    wave_sync();
    for (int i = lane; i < nc; i += 64) lamv[i] = 0.0;
    wave_sync();
    if (st == QP_OPTIMAL)
        for (int i = lane; i < nc; i += 64) { const int v = lp.rowvar[i]; if (v < nc) lamv[v] = lp.T[(size_t)i * lp.ld]; }
    wave_sync();
}

// LDS view of the k_qp_batch tableau: (nc + 1) x ld doubles, the index block, then nc multipliers
__device__ inline double *qp_lds_layout(Lp &lp, double *smem, int nc, int ld) {
    int *ib = reinterpret_cast<int *>(smem + (size_t)(nc + 1) * ld);
    lp.T = smem; lp.ld = ld; lp.colvar = ib; lp.rowvar = ib + ld + 1; lp.rowkind = ib + ld + 1 + nc + 2;
    // (ld + 1) + 2 (nc + 2) ints precede it and ld is odd: the int block has an even length, lamv is 8-byte aligned as it stands
    return reinterpret_cast<double *>(lp.rowkind + nc + 2);
}

__global__ void __launch_bounds__(64) k_qp_batch(long long n_qp, int nc, int n_eq, int nt, int nx, int ld, const double *__restrict__ W,
                                                 const double *__restrict__ UV, const double *__restrict__ X0H, const double *__restrict__ Gt,
                                                 const double *__restrict__ theta, int32_t *__restrict__ status, double *__restrict__ x,
                                                 double *__restrict__ lam, uint8_t *__restrict__ active, int32_t *__restrict__ iters,
                                                 unsigned int *work) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = lane_id(), nr = nt + 1;
    Lp lp;
    double *lamv = qp_lds_layout(lp, smem, nc, ld);   // multipliers of the solved point
    for (;;) {
        unsigned int w = 0;
        if (lane == 0) w = atomicAdd(work, 1u);
        w = (unsigned)__builtin_amdgcn_readfirstlane((int)w);
        if (w >= n_qp) break;
        const double *th = theta + (size_t)w * nt;
        qp_lcp_dict(lp, nc, n_eq, W, lamv, [&](int i) {
            double q = UV[(size_t)i * nr];
            for (int t = 0; t < nt; ++t) q = fma(UV[(size_t)i * nr + 1 + t], th[t], q);
            return q;
        });
        const int st = qp_lemke(lp, nc, n_eq);
        // outputs
        qp_multipliers(lp, nc, st, lamv);
        if (lam) for (int i = lane; i < nc; i += 64) lam[(size_t)w * nc + i] = lamv[i];
        if (active) {
            // a constraint is active when its slack is nonbasic (zero) in the final dictionary
            for (int i = lane; i < nc; i += 64) active[(size_t)w * nc + i] = st == QP_OPTIMAL ? 1 : 0;
            wave_sync();
            if (st == QP_OPTIMAL)
                for (int i = lane; i < nc; i += 64) { const int v = lp.rowvar[i]; if (v >= nc && v < 2 * nc) active[(size_t)w * nc + (v - nc)] = 0; }
        }
        if (x) {
            for (int a = lane; a < nx; a += 64) {
                double v = X0H[(size_t)a * nr];
                for (int t = 0; t < nt; ++t) v = fma(X0H[(size_t)a * nr + 1 + t], th[t], v);
                for (int i = 0; i < nc; ++i) v = fma(-lamv[i], Gt[(size_t)i * nx + a], v);
                x[(size_t)w * nx + a] = st == QP_OPTIMAL ? v : __longlong_as_double(0x7ff8000000000000ll);
            }
        }
        if (lane == 0) { status[w] = st; if (iters) iters[w] = lp.iters; }
        wave_sync();
    }
}

// ---- the MIQP at fixed parameter points: one LCP per (point, binary fixation) pair ------------------------------------------
// With the binaries y fixed, the continuous QP of an MIQP keeps its Hessian Q_c and its constraint rows A_c; only the right-hand
// side and the linear term move, both affine in z = [1; theta; y].  So every pair shares W = A_c Q_c^-1 A_c' and only
// q = UV z changes (the host assembly: MPMIQP_Program.theta_blocks).  Rows without continuous content but with theta content
// are check rows: s = CK z decides them alone (s >= -MIQP_CHECK_TOL, or |s| <= MIQP_CHECK_TOL on equality rows).
constexpr double MIQP_CHECK_TOL = MPC_MIQP_CHECK_TOL;   // include/mpcombi.h

struct MiqpBlocks {
    int nc, n_eq, nxc, nt, nb, nz, n_ck, n_x, n_rows;
    const double *W, *UV, *X0, *Gt, *Qc, *G, *K, *CK, *Y, *theta;
    const uint8_t *ck_eq;
    const int32_t *cont_idx, *bin_idx, *lcp_row;
};

// LDS: the k_qp_batch tableau and multipliers, then z (nz) and x (nxc)
__device__ inline int miqp_pair(const MiqpBlocks &B, Lp &lp, double *lamv, long long p, long long leaf, double &obj) {
    const int lane = lane_id(), nz = B.nz, nc = B.nc, nxc = B.nxc;
    double *zv = lamv + nc, *xv = zv + nz;
    for (int k = lane; k < nz; k += 64)
        zv[k] = k == 0 ? 1.0 : (k <= B.nt ? B.theta[(size_t)p * B.nt + k - 1] : B.Y[(size_t)leaf * B.nb + k - 1 - B.nt]);
    wave_sync();
    int bad = 0;
    for (int k = lane; k < B.n_ck; k += 64) {
        const double *ck = B.CK + (size_t)k * nz;
        double s = ck[0];
        for (int j = 1; j < nz; ++j) s = fma(ck[j], zv[j], s);
        if (B.ck_eq[k] ? !(fabs(s) <= MIQP_CHECK_TOL) : !(s >= -MIQP_CHECK_TOL)) bad = 1;
    }
    obj = __longlong_as_double(0x7ff8000000000000ll);
    if (wave_max_i(bad)) return QP_INFEASIBLE;                     // a violated check row: no pivot
    qp_lcp_dict(lp, nc, B.n_eq, B.W, lamv, [&](int i) {
        const double *u = B.UV + (size_t)i * nz;
        double q = u[0];
        for (int j = 1; j < nz; ++j) q = fma(u[j], zv[j], q);
        return q;
    });
    const int st = qp_lemke(lp, nc, B.n_eq);
    qp_multipliers(lp, nc, st, lamv);
    if (st != QP_OPTIMAL) return st;
    // x = X0 z - Gt' lambda
    for (int a = lane; a < nxc; a += 64) {
        double v = B.X0[(size_t)a * nz];
        for (int j = 1; j < nz; ++j) v = fma(B.X0[(size_t)a * nz + j], zv[j], v);
        for (int i = 0; i < nc; ++i) v = fma(-lamv[i], B.Gt[(size_t)i * nxc + a], v);
        xv[a] = v;
    }
    wave_sync();
    // objective 1/2 x'Q_c x + (G z)'x + 1/2 z'K z: a term per lane, one butterfly sum, lane 0's total for every lane
    double part = 0.0;
    for (int a = lane; a < nxc; a += 64) {
        double qx = 0.0, gz = B.G[(size_t)a * nz];
        for (int b = 0; b < nxc; ++b) qx = fma(B.Qc[(size_t)a * nxc + b], xv[b], qx);
        for (int j = 1; j < nz; ++j) gz = fma(B.G[(size_t)a * nz + j], zv[j], gz);
        part += xv[a] * (0.5 * qx + gz);
    }
    for (int k = lane; k < nz; k += 64) {
        double kz = 0.0;
        for (int j = 0; j < nz; ++j) kz = fma(B.K[(size_t)k * nz + j], zv[j], kz);
        part += 0.5 * zv[k] * kz;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    obj = __shfl(part, 0);
    return st;
}

// pass 1: (status, objective) of every (point, leaf) pair, [points x leaves]
__global__ void __launch_bounds__(64) k_miqp_pairs(MiqpBlocks B, long long m, long long n_leaves, int ld, int32_t *__restrict__ status,
                                                   double *__restrict__ obj, unsigned int *work) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    Lp lp;
    double *lamv = qp_lds_layout(lp, smem, B.nc, ld);
    const long long n_pairs = m * n_leaves;
    for (;;) {
        unsigned long long w = 0;
        if (lane_id() == 0) w = atomicAdd(reinterpret_cast<unsigned long long *>(work), 1ull);
        w = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(w >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)w);
        if (w >= (unsigned long long)n_pairs) break;
        double f;
        const int st = miqp_pair(B, lp, lamv, (long long)(w / n_leaves), (long long)(w % n_leaves), f);
        if (lane_id() == 0) { status[w] = st; obj[w] = f; }
        wave_sync();
    }
}

// pick pass, one thread per point: the lowest objective among the optimal pairs, the lowest leaf on ties (Solver.solve_milp).
// A point with an iteration-limited pair is reported as such (its minimum is not certain); with no optimal pair it is infeasible.
__global__ void k_miqp_pick(long long m, long long n_leaves, const int32_t *__restrict__ status, const double *__restrict__ obj,
                            int32_t *__restrict__ pst, int32_t *__restrict__ leaf, double *__restrict__ best) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    long long bl = -1;
    double bo = 0.0;
    bool lim = false;
    for (long long l = 0; l < n_leaves; ++l) {
        const int s = status[p * n_leaves + l];
        if (s == QP_ITERLIMIT) lim = true;
        if (s != QP_OPTIMAL) continue;
        const double o = obj[p * n_leaves + l];
        if (bl < 0 || o < bo) { bl = l; bo = o; }
    }
    pst[p] = lim ? QP_ITERLIMIT : (bl >= 0 ? QP_OPTIMAL : QP_INFEASIBLE);
    leaf[p] = lim ? -1 : (int32_t)bl;
    best[p] = bl >= 0 && !lim ? bo : __longlong_as_double(0x7ff8000000000000ll);
}

// winner pass: each point's winning pair once more (the same arithmetic as pass 1), writing x (y spliced in), the multipliers
// over all program rows and the active flags of the LCP rows
__global__ void __launch_bounds__(64) k_miqp_winners(MiqpBlocks B, long long m, int ld, const int32_t *__restrict__ leaf,
                                                     double *__restrict__ obj, double *__restrict__ x, double *__restrict__ lam,
                                                     uint8_t *__restrict__ active, unsigned int *work) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    Lp lp;
    double *lamv = qp_lds_layout(lp, smem, B.nc, ld);
    const int lane = lane_id(), nc = B.nc;
    const double *xv = lamv + nc + B.nz;
    for (;;) {
        unsigned int w = 0;
        if (lane == 0) w = atomicAdd(work, 1u);
        w = (unsigned)__builtin_amdgcn_readfirstlane((int)w);
        if (w >= m) break;
        const long long l = leaf[w];
        if (l < 0) continue;
        double f;
        const int st = miqp_pair(B, lp, lamv, w, l, f);
        if (lane == 0) obj[w] = st == QP_OPTIMAL ? f : __longlong_as_double(0x7ff8000000000000ll);
        if (x) {
            for (int a = lane; a < B.nxc; a += 64) x[(size_t)w * B.n_x + B.cont_idx[a]] = xv[a];
            for (int k = lane; k < B.nb; k += 64) x[(size_t)w * B.n_x + B.bin_idx[k]] = B.Y[(size_t)l * B.nb + k];
        }
        if (lam) for (int i = lane; i < nc; i += 64) lam[(size_t)w * B.n_rows + B.lcp_row[i]] = lamv[i];
        if (active) {
            // as in k_qp_batch: a row is active when its slack is nonbasic in the final dictionary
            for (int i = lane; i < nc; i += 64) active[(size_t)w * B.n_rows + B.lcp_row[i]] = st == QP_OPTIMAL ? 1 : 0;
            wave_sync();
            for (int i = lane; i < nc; i += 64) { const int v = lp.rowvar[i]; if (v >= nc && v < 2 * nc) active[(size_t)w * B.n_rows + B.lcp_row[v - nc]] = 0; }
        }
        wave_sync();
    }
}

}  // namespace mpc
