// simplex.hpp -- the wavefront vertex simplex in LDS shared by the search-tree classifier (tree.hpp) and the region merger
// (merge.hpp); DESIGN §3.13, §3.14.
//
// The simplex (tr_simplex): the working set holds n_t "rows", real rows of P^_j or pseudo rows (fixed coordinates, free to move either
// way), with the columns of the inverse basis d_k in LDS (B d_k = e_k).  Slot k's rate mu_k = c.d_k; a pseudo slot enters when
// |mu_k| / |d_k| > 1e-11, a real slot when mu_k / |d_k| > 1e-11 (the largest normalised rate first, pseudo slots before real ones).
// Ratio test over the rows outside the set (lanes over rows, slacks clamped at 0), ties to the lowest row; no blocking row: unbounded.
// A row blocks when its rate along the direction p = -+d_k exceeds 1e-12 max(1, |p|), not 1e-12 alone: next to a nearly parallel row in
// the set |d_k| reaches 1e5, and the rate of an exact copy of a working row (the rows of a merged region and of its member stacked, as
// Solution.compare does) is then rounding noise of 1e-11 instead of 0; taken as a blocking row at step 0 it was a pivot of 1e-12 that
// left the inverse basis without meaning (a radius of -1.7e-12 for 0.034, and one of 0.045 at an infeasible point for -0.37).
// A run that reaches TR_PIVOT_CAP pivots reports "unbounded" as well: a wider bound than the true one never costs exactness.
// Column n_t of a row is the coefficient of the extra coordinate of a (theta, t) run (d = n_t + 1): tr_load sets it to -1 for phase 1,
// other loaders set their own.  ``stop_t`` ends a run of dimension n_t + 1 as soon as x_{n_t} exceeds it (TR_REACHED).
#pragma once
#include <stdint.h>

namespace mpc {

constexpr int TR_MAX_NT = 16, TR_MAX_ROWS = 256, TR_D = TR_MAX_NT + 1, TR_PIVOT_CAP = 400;
constexpr double TR_RATE_EPS = 1e-11, TR_RATE_G = 1e-12, TR_PHASE1_EPS = 1e-9;

// LDS of one wavefront (workgroup of 64): rows A[m][n_t + 1] (column n_t = -1 for phase 1), b[m], flags, inverse basis, state
struct TrLds {
    double *A, *b, *D, *x, *p, *c, *box;   // D: [TR_D][TR_D], slot k at D[k * TR_D + i]; box: [2][TR_D] lower, upper
    int *flag, *W;                         // flag[r]: 0 free row, 1 in the working set, 2 dropped (zero row)
};

__host__ __device__ inline size_t tr_lds_bytes(int m_max, int nt) {
    return (size_t)m_max * (nt + 2) * 8 + (size_t)(TR_D * TR_D + 5 * TR_D) * 8 + (size_t)(m_max + TR_D) * 4;
}

__device__ inline TrLds tr_lds(double *base, int m_max, int nt) {
    TrLds S;
    S.A = base;
    S.b = S.A + (size_t)m_max * (nt + 1);
    S.D = S.b + m_max;
    S.x = S.D + TR_D * TR_D;
    S.p = S.x + TR_D;
    S.c = S.p + TR_D;
    S.box = S.c + TR_D;
    S.flag = reinterpret_cast<int *>(S.box + 2 * TR_D);
    S.W = S.flag + m_max;
    return S;
}

// the unit rows of P^_j: a = E_i / |E_i|, b = (f_i + tol max(1, |E_i|)) / |E_i|; a zero row is dropped (or empties the set).
// Returns 1 when a zero row empties the polytope.
__device__ inline int tr_load(const TrLds &S, const double *ef, long long r0, int m, int nt, double tol) {
    const int lane = threadIdx.x & 63;
    int empty = 0;
    for (int i = lane; i < m; i += 64) {
        const double *row = ef + (r0 + i) * (long long)(nt + 1);
        double nn = 0.0;
        for (int t = 0; t < nt; ++t) nn = fma(row[1 + t], row[1 + t], nn);
        const double nrm = sqrt(nn), rhs = row[0] + tol * fmax(1.0, nrm);
        if (nrm == 0.0) {
            S.flag[i] = 2;
            if (rhs < 0.0) empty = 1;
            for (int t = 0; t <= nt; ++t) S.A[i * (nt + 1) + t] = 0.0;
            S.b[i] = 0.0;
        } else {
            S.flag[i] = 0;
            for (int t = 0; t < nt; ++t) S.A[i * (nt + 1) + t] = row[1 + t] / nrm;
            S.A[i * (nt + 1) + nt] = -1.0;
            S.b[i] = rhs / nrm;
        }
    }
    __syncthreads();
    return __any(empty) ? 1 : 0;
}

// working set of pseudo rows at the current point: D = I (dimension d), W = -1, no row in the set
__device__ inline void tr_reset_basis(const TrLds &S, int m, int d) {
    const int lane = threadIdx.x & 63;
    if (lane < TR_D) {
        S.W[lane] = -1;
        for (int i = 0; i < TR_D; ++i) S.D[lane * TR_D + i] = (i == lane && lane < d) ? 1.0 : 0.0;
    }
    for (int i = lane; i < m; i += 64) if (S.flag[i] == 1) S.flag[i] = 0;
    __syncthreads();
}

enum { TR_OPTIMAL = 0, TR_UNBOUNDED = 1, TR_CAPPED = 2, TR_REACHED = 3 };

// minimise S.c . x over the rows from the current point and working set.  d = n_t (phase 2) or n_t + 1 (phase 1: c = e_{n_t},
// the run ends as soon as x_{n_t} reaches 0; or a (theta, t) run that ends once x_{n_t} > stop_t).  x moves only to feasible points; on UNBOUNDED / CAPPED x is the last point reached.
__device__ inline int tr_simplex(const TrLds &S, int m, int nt, int d, bool phase1, unsigned long long &pivots,
                                 double stop_t = INFINITY) {
    const int lane = threadIdx.x & 63, stride = nt + 1;
    for (int it = 0; it < TR_PIVOT_CAP; ++it) {
        if (d > nt && S.x[nt] > stop_t) return TR_REACHED;   // S.x is settled: every iteration ends with a barrier
        // 1. entering slot
        double key = -1.0, sgn = 1.0, dd = 0.0;
        int slot = -1;
        if (lane < d) {
            double mu = 0.0;
            for (int i = 0; i < d; ++i) { const double v = S.D[lane * TR_D + i]; mu = fma(S.c[i], v, mu); dd = fma(v, v, dd); }
            const double rate = dd > 0.0 ? mu / sqrt(dd) : 0.0;
            if (S.W[lane] < 0) { if (fabs(rate) > TR_RATE_EPS) { key = 4.0 + fabs(rate); slot = lane; sgn = rate > 0.0 ? 1.0 : -1.0; } }
            else if (rate > TR_RATE_EPS) { key = rate; slot = lane; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ok = __shfl_xor(key, off);
            const int os = __shfl_xor(slot, off);
            if (os >= 0 && (slot < 0 || ok > key || (ok == key && os < slot))) { key = ok; slot = os; }
        }
        if (slot < 0) return TR_OPTIMAL;
        sgn = __shfl(sgn, slot);
        const double g_min = TR_RATE_G * fmax(1.0, sqrt(__shfl(dd, slot)));   // relative to |p| = |d_slot| (the header comment)
        // 2. direction p = -sgn d_slot
        if (lane < d) S.p[lane] = -sgn * S.D[slot * TR_D + lane];
        __syncthreads();
        // 3. ratio test (ties to the lowest row; -2: phase 1 reaches x_{n_t} = 0, preferred on a tie)
        double tbest = INFINITY;
        int rbest = -1;
        for (int r = lane; r < m; r += 64) {
            if (S.flag[r]) continue;
            double g = 0.0, ax = 0.0;
            for (int i = 0; i < d; ++i) { const double a = S.A[r * stride + i]; g = fma(a, S.p[i], g); ax = fma(a, S.x[i], ax); }
            if (g > g_min) {
                const double t = fmax(S.b[r] - ax, 0.0) / g;
                if (t < tbest || (t == tbest && r < rbest)) { tbest = t; rbest = r; }
            }
        }
        if (phase1 && lane == 0 && S.p[nt] < 0.0) {
            const double t = S.x[nt] / -S.p[nt];
            if (t <= tbest) { tbest = t; rbest = -2; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ot = __shfl_xor(tbest, off);
            const int orow = __shfl_xor(rbest, off);
            if (orow != -1 && (rbest == -1 || ot < tbest || (ot == tbest && orow < rbest))) { tbest = ot; rbest = orow; }
        }
        if (rbest == -1) return TR_UNBOUNDED;
        // 4. move
        __syncthreads();
        if (lane < d) S.x[lane] = fma(tbest, S.p[lane], S.x[lane]);
        if (rbest == -2) {
            if (lane == 0) S.x[nt] = 0.0;
            __syncthreads();
            return TR_REACHED;
        }
        // 5. row rbest replaces the slot: d_k' = d_k / alpha_k, d_j' = d_j - alpha_j d_k'
        double dk[TR_D];
        double alpha = 0.0;
#pragma unroll
        for (int i = 0; i < TR_D; ++i) dk[i] = i < d ? S.D[slot * TR_D + i] : 0.0;
        if (lane < d)
            for (int i = 0; i < d; ++i) alpha = fma(S.A[rbest * stride + i], S.D[lane * TR_D + i], alpha);
        const double ak = __shfl(alpha, slot);
        __syncthreads();
        if (lane < d) {
#pragma unroll
            for (int i = 0; i < TR_D; ++i) {
                if (i >= d) continue;
                const double nk = dk[i] / ak;
                S.D[lane * TR_D + i] = lane == slot ? nk : fma(-alpha, nk, S.D[lane * TR_D + i]);
            }
        }
        if (lane == 0) {
            const int old = S.W[slot];
            if (old >= 0) S.flag[old] = 0;
            S.flag[rbest] = 1;
            S.W[slot] = rbest;
        }
        __syncthreads();
        ++pivots;
    }
    return TR_CAPPED;
}

// a feasible point of the rows (phase 1 from theta = 0 in (theta, t) with rows a.theta - t <= b), left in x[0..nt) with a fresh
// phase-2 working set; returns false when the polytope is empty (min t > TR_PHASE1_EPS, or the run was capped)
__device__ inline bool tr_feasible(const TrLds &S, int m, int nt, unsigned long long &pivots) {
    const int lane = threadIdx.x & 63;
    double worst = 0.0;
    for (int r = lane; r < m; r += 64) if (!S.flag[r]) worst = fmax(worst, -S.b[r]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) worst = fmax(worst, __shfl_xor(worst, off));
    if (lane < TR_D) { S.x[lane] = lane == nt ? worst : 0.0; S.c[lane] = lane == nt ? 1.0 : 0.0; }
    __syncthreads();
    bool ok = true;
    if (worst > 0.0) {
        tr_reset_basis(S, m, nt + 1);
        const int st = tr_simplex(S, m, nt, nt + 1, true, pivots);
        ok = st == TR_REACHED || (st == TR_OPTIMAL && S.x[nt] <= TR_PHASE1_EPS);
        __syncthreads();
        if (lane == 0) S.x[nt] = 0.0;
    }
    tr_reset_basis(S, m, nt);
    return ok;
}

__device__ inline double tr_dot_x(const TrLds &S, int nt) {
    double v = 0.0;
    for (int t = 0; t < nt; ++t) v = fma(S.c[t], S.x[t], v);
    return v;
}

// c = sign * plane normal (lanes t < nt), then min c.x; returns min or -inf
__device__ inline double tr_min_plane(const TrLds &S, const double *nrm, double sign, int m, int nt, unsigned long long &pivots,
                                      unsigned long long &capped) {
    const int lane = threadIdx.x & 63;
    __syncthreads();
    if (lane < TR_D) S.c[lane] = lane < nt ? sign * nrm[lane] : 0.0;
    __syncthreads();
    const int st = tr_simplex(S, m, nt, nt, false, pivots);
    if (st == TR_CAPPED) ++capped;
    return st == TR_OPTIMAL ? tr_dot_x(S, nt) : -INFINITY;
}

// the bounding box of the loaded rows from the current feasible point: 2 n_t LPs, lower bounds in box[0 .. n_t), upper bounds in
// box[TR_D ..); an unbounded or capped run gives -inf / +inf
__device__ inline void tr_box(const TrLds &S, int m, int nt, unsigned long long &pivots, unsigned long long &capped, unsigned long long &lps) {
    const int lane = threadIdx.x & 63;
    for (int t = 0; t < nt; ++t) {
        __syncthreads();
        if (lane < TR_D) S.c[lane] = lane == t ? 1.0 : 0.0;
        __syncthreads();
        int st = tr_simplex(S, m, nt, nt, false, pivots);
        capped += st == TR_CAPPED;
        const double lo = st == TR_OPTIMAL ? S.x[t] : -INFINITY;
        __syncthreads();
        if (lane < TR_D) S.c[lane] = lane == t ? -1.0 : 0.0;
        __syncthreads();
        st = tr_simplex(S, m, nt, nt, false, pivots);
        capped += st == TR_CAPPED;
        const double hi = st == TR_OPTIMAL ? S.x[t] : INFINITY;
        if (lane == 0) { S.box[t] = lo; S.box[TR_D + t] = hi; }
        lps += 2;
    }
    __syncthreads();
}

}  // namespace mpc
