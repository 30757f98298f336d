// transition.hpp -- the LPs of Solution.transition_graph (gfx950): image boxes and the pair stage; DESIGN §3.20.
//
// Regions arrive as unit rows [o | n] (|n| = 1, R = {theta : n.theta <= o}), at most OV_MAX_ROWS each; region i carries the closed-loop
// map theta+ = Phi_i theta + phi_i.  Every LP is a run of the wavefront vertex simplex of simplex.hpp over rows in LDS; one WAVEFRONT
// (workgroup of 64) per item.
//
//   k_transition_boxes  one wavefront per region i: the rows of R_i in LDS and, from xs[i] (a feasible point, of k_merge_regions), the
//                       exact bounding box of the image Phi_i R_i + phi_i: 2 n_t runs of tr_min_plane with the rows of Phi_i as
//                       objectives, each warm-started from the one before.  An unbounded run gives -inf / +inf; a capped one too, and
//                       sets flag[i].
//   k_transition_pairs  one wavefront per candidate pair (i, j): the rows of R_i, then the rows of R_j pulled back through the map of i.
//     pulled-back row   [o | n] of R_j becomes a.theta <= beta with a = Phi_i^T n, beta = o - n.phi_i, s = |a|.  With
//                       s > TS_ROW_EPS max(1, max |Phi_i|) the LDS row is the unit row [beta / s | a / s]; otherwise the row is constant:
//                       beta < -tol empties T_ij (radius -inf, no LP), else the row is dropped (flag 2, which the ratio test skips; its
//                       right-hand side is +inf, which the smallest slack skips).
//     radius run        ov_radius over the m_i + m_j rows from xs[i]: to the optimum (full_radius) or until t > tol (TR_REACHED; the
//                       radius is then a lower bound above tol).
//     output            radius[k], status[k] (TS_NO_EDGE: r <= tol, TS_EDGE, TS_UNBOUNDED: radius +inf, TS_UNDECIDED: the run stopped
//                       at the pivot cap, radius is the t it reached) and witness[k][n_t], the theta where the run ended (an unbounded
//                       run that ended with t < 2 tol is moved along its ray to t = 2 tol).
//   The only atomics are the counters; no floating-point atomics: a rerun gives the same bits.
#pragma once
#include <stdint.h>

#include "overlap.hpp"

namespace mpc {

constexpr double TS_ROW_EPS = 1e-12;
enum { TS_NO_EDGE = 0, TS_EDGE = 1, TS_UNBOUNDED = 2, TS_UNDECIDED = 3 };

__global__ void __launch_bounds__(64) k_transition_boxes(int nt, int m_max, long long n_regions, const long long *__restrict__ row_off,
                                                         const double *__restrict__ ef, const double *__restrict__ Phi,
                                                         const double *__restrict__ phi, const double *__restrict__ xs,
                                                         double *__restrict__ box, int32_t *__restrict__ flag,
                                                         unsigned long long *__restrict__ counters) {
    extern __shared__ double ts_smem[];
    const int lane = threadIdx.x & 63;
    const long long i = blockIdx.x;
    if (i >= n_regions) return;
    const TrLds S = tr_lds(ts_smem, m_max, nt);
    const long long r0 = row_off[i];
    const int m = (int)(row_off[i + 1] - r0);
    unsigned long long pivots = 0, capped = 0;
    ov_load(S, ef, r0, m, nt, 0);
    if (lane < TR_D) S.x[lane] = lane < nt ? xs[i * nt + lane] : 0.0;
    __syncthreads();
    tr_reset_basis(S, m, nt);
    const double *P = Phi + i * (long long)nt * nt;
    for (int t = 0; t < nt; ++t) {
        const double lo = tr_min_plane(S, P + t * nt, 1.0, m, nt, pivots, capped) + phi[i * nt + t];
        const double hi = -tr_min_plane(S, P + t * nt, -1.0, m, nt, pivots, capped) + phi[i * nt + t];
        if (lane == 0) {
            box[(2 * i) * nt + t] = lo;
            box[(2 * i + 1) * nt + t] = hi;
        }
    }
    if (lane == 0) {
        flag[i] = capped ? 1 : 0;
        atomicAdd(counters + 0, 2ull * nt);
        atomicAdd(counters + 1, pivots);
        atomicAdd(counters + 2, capped);
    }
}

// the m_j rows of a target region (rows [r0_j, r0_j + m_j) of ef) pulled back through theta+ = P theta + sh into the LDS rows
// [at, at + m_j), lanes over rows: unit rows, or flag 2 with right-hand side +inf for a constant row (the header comment).  Returns, per
// lane, 1 where a constant row of that lane empties the pulled-back set (the caller votes with __any); no barrier.
__device__ inline int ts_pull_back(const TrLds &S, const double *ef, long long r0_j, int m_j, int nt, int at, const double *P, const double *sh,
                                   double tol) {
    const int lane = threadIdx.x & 63, nr = nt + 1;
    double big = 0.0;
    for (int e = lane; e < nt * nt; e += 64) big = fmax(big, fabs(P[e]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) big = fmax(big, __shfl_xor(big, off));
    const double thr = TS_ROW_EPS * fmax(1.0, big);
    int empty = 0;
    for (int r = lane; r < m_j; r += 64) {
        const double *row = ef + (r0_j + r) * (long long)nr;
        double *out = S.A + (size_t)(at + r) * nr;
        double beta = row[0], ss = 0.0;
        for (int t = 0; t < nt; ++t) beta = fma(-row[1 + t], sh[t], beta);
        for (int k = 0; k < nt; ++k) {
            double v = 0.0;
            for (int t = 0; t < nt; ++t) v = fma(P[t * nt + k], row[1 + t], v);
            out[k] = v;
            ss = fma(v, v, ss);
        }
        const double s = sqrt(ss);
        if (s > thr) {
            for (int k = 0; k < nt; ++k) out[k] /= s;
            out[nt] = 1.0;
            S.b[at + r] = beta / s;
            S.flag[at + r] = 0;
        } else {
            if (beta < -tol) empty = 1;
            for (int k = 0; k <= nt; ++k) out[k] = 0.0;
            S.b[at + r] = INFINITY;
            S.flag[at + r] = 2;
        }
    }
    return empty;
}

struct TransitionPairArgs {
    int nt, m_max, full_radius;      // m_max: LDS rows, at least m_i + m_j of every pair
    long long n_pairs;
    const long long *row_off;
    const double *ef;                // [rows][nt + 1] unit [o | n]
    const double *Phi, *phi;         // [n_regions][nt][nt], [n_regions][nt]
    const double *xs;                // [n_regions][nt] where the radius run of a pair starts (region i's row)
    const int32_t *pair_a, *pair_b;
    double tol;
    double *radius, *witness;        // witness [n_pairs][nt]
    int32_t *status;
    unsigned long long *counters;    // pairs, LPs, pivots, capped
};

__global__ void __launch_bounds__(64) k_transition_pairs(TransitionPairArgs a) {
    extern __shared__ double ts_smem[];
    const int lane = threadIdx.x & 63, nt = a.nt;
    const long long q = blockIdx.x;
    if (q >= a.n_pairs) return;
    const TrLds S = tr_lds(ts_smem, a.m_max, nt);
    const long long reg_i = a.pair_a[q], reg_j = a.pair_b[q], r0_i = a.row_off[reg_i], r0_j = a.row_off[reg_j];
    const int m_i = (int)(a.row_off[reg_i + 1] - r0_i), m_j = (int)(a.row_off[reg_j + 1] - r0_j), m = m_i + m_j;
    const double *P = a.Phi + reg_i * (long long)nt * nt, *sh = a.phi + reg_i * nt;
    unsigned long long pivots = 0, lps = 0;
    ov_load(S, a.ef, r0_i, m_i, nt, 0);
    const int empty = ts_pull_back(S, a.ef, r0_j, m_j, nt, m_i, P, sh, a.tol);
    double r = -INFINITY;
    int status = TS_NO_EDGE;
    if (lane < TR_D) S.x[lane] = lane < nt ? a.xs[reg_i * nt + lane] : 0.0;
    if (!__any(empty)) {
        const int st = ov_radius(S, m, nt, a.full_radius ? INFINITY : a.tol, pivots);
        lps = 1;
        r = S.x[nt];
        if (st == TR_UNBOUNDED) {
            // no row blocks the direction S.p, along which t grows: the witness moves on until t = 2 tol
            const double rate = S.p[nt], step = (r < 2.0 * a.tol && rate > 0.0) ? (2.0 * a.tol - r) / rate : 0.0;
            __syncthreads();
            if (lane < nt) S.x[lane] = fma(step, S.p[lane], S.x[lane]);
            r = INFINITY;
            status = TS_UNBOUNDED;
        } else if (st == TR_CAPPED) {
            status = TS_UNDECIDED;
        } else {
            status = r > a.tol ? TS_EDGE : TS_NO_EDGE;
        }
    }
    __syncthreads();
    if (lane < nt) a.witness[q * nt + lane] = S.x[lane];
    if (lane == 0) {
        a.radius[q] = r;
        a.status[q] = status;
        atomicAdd(a.counters + 0, 1ull);
        atomicAdd(a.counters + 1, lps);
        atomicAdd(a.counters + 2, pivots);
        atomicAdd(a.counters + 3, status == TS_UNDECIDED ? 1ull : 0ull);
    }
}

}  // namespace mpc
