// reduce.hpp -- removing the redundant rows of polytopes (gfx950): one radius run per row; DESIGN §3.22.
//
// A polytope arrives as unit rows [o | n] (|n| = 1, {theta : n.theta <= o}), at most RD_MAX_ROWS of them, in order.  Every LP is a radius
// run (ov_radius, overlap.hpp) of the wavefront vertex simplex of simplex.hpp over rows in LDS; one WAVEFRONT (workgroup of 64) per polytope.
//
//   k_reduce_rows  LDS rows [0, m): the polytope P.
//     thin test    radius(P) from the item's start point (the origin without one), the run stops once t > tol.  Optimal with t <= tol: P
//                  is THIN, every mask bit is set and no row is tested.  Otherwise the theta where the run ended is kept in registers (lane
//                  i holds theta_i) and every row run starts there, so a row's verdict depends on the live rows and on k alone, not on the
//                  path of the runs before it.
//     row loop     in place, k = 0 .. m - 1 in order.  Row k is read from slot k and written reversed into the same slot (-n, -o), then
//                  the radius over all m slots, the run stops once t > tol: the rows still live and {n_k.theta >= o_k}.  Optimal with
//                  t <= tol: row k is redundant, its slot becomes a dropped row (flag 2, right-hand side +inf, the convention of
//                  ts_pull_back: the ratio test and the smallest slack skip it, tr_reset_basis never clears it) and bounds no later run.
//                  Otherwise the slot is turned forward again, bit for bit the loaded values, and mask bit k is set.  A run that is
//                  unbounded or stopped at the pivot cap counts as "kept" and is counted in wide: the reduced polytope never loses a
//                  state of P.
//     output       status[q]: RD_OK or RD_THIN; wide[q]: the unbounded or capped runs; kept[q][RD_WORDS]: bit k, row k stays;
//                  point[q][n_t] (optional): the saved point, a start point for later calls.
//   The only atomics are the counters; no floating-point atomics: a rerun gives the same bits.
#pragma once
#include <stdint.h>

#include "overlap.hpp"

namespace mpc {

constexpr int RD_MAX_ROWS = 512, RD_WORDS = RD_MAX_ROWS / 64;
enum { RD_OK = 0, RD_THIN = 1 };

struct ReduceArgs {
    int nt, m_max;                        // m_max: LDS rows, at least the rows of every polytope
    long long n_poly;
    const long long *row_off;
    const double *ef;                     // unit [o | n]
    const double *start;                  // [n_poly][nt] where the thin test starts, or nullptr: the origin
    double tol;
    int32_t *status, *wide;
    unsigned long long *kept;             // [n_poly][RD_WORDS]
    double *point;                        // [n_poly][nt], or nullptr
    unsigned long long *counters;         // polytopes, thin ones, LPs, pivots, unbounded or capped runs
};

// The row loop of the header comment over the LDS rows [0, m), every run started from px (lane i holds theta_i): kept bit k is set for
// a row that stays.  SKIP_DROPPED: a slot that is a dropped row already (flag 2, a constant row of ts_pull_back; k_reduce_rows has
// none) is passed over without an LP and without a bit.  s_kept is zeroed by the caller; no barrier behind the last row.
template <bool SKIP_DROPPED>
__device__ inline void rd_row_loop(const TrLds &S, int m, int nt, double tol, double px, unsigned long long &pivots, unsigned long long &lps,
                                   unsigned long long &wide, unsigned long long *s_kept) {
    const int lane = threadIdx.x & 63, nr = nt + 1;
    for (int k = 0; k < m; ++k) {
        __syncthreads();
        if (SKIP_DROPPED && S.flag[k] == 2) continue;
        const double v = lane < nt ? S.A[k * nr + lane] : 0.0, rhs = S.b[k];
        __syncthreads();
        if (lane < nt) { S.A[k * nr + lane] = -v; S.x[lane] = px; }
        if (lane == 0) { S.b[k] = -rhs; S.flag[k] = 0; }
        const int st = ov_radius(S, m, nt, tol, pivots);
        ++lps;
        wide += st == TR_UNBOUNDED || st == TR_CAPPED;
        const bool redundant = st == TR_OPTIMAL && !(S.x[nt] > tol);
        __syncthreads();
        if (redundant) {
            if (lane <= nt) S.A[k * nr + lane] = 0.0;
            if (lane == 0) { S.b[k] = INFINITY; S.flag[k] = 2; }
        } else {
            if (lane < nt) S.A[k * nr + lane] = v;
            if (lane == 0) { S.b[k] = rhs; s_kept[k >> 6] |= 1ull << (k & 63); }
        }
    }
}

__global__ void __launch_bounds__(64) k_reduce_rows(ReduceArgs a) {
    extern __shared__ double rd_smem[];
    __shared__ unsigned long long s_kept[RD_WORDS];
    const int lane = threadIdx.x & 63, nt = a.nt;
    const long long q = blockIdx.x;
    if (q >= a.n_poly) return;
    const TrLds S = tr_lds(rd_smem, a.m_max, nt);
    const long long r0 = a.row_off[q];
    const int m = (int)(a.row_off[q + 1] - r0);
    const double tol = a.tol;
    unsigned long long pivots = 0, wide = 0, lps = 1;
    ov_load(S, a.ef, r0, m, nt, 0);
    if (lane < TR_D) S.x[lane] = (lane < nt && a.start) ? a.start[q * nt + lane] : 0.0;
    if (lane < RD_WORDS) s_kept[lane] = 0ull;
    int st = ov_radius(S, m, nt, tol, pivots);
    wide += st == TR_UNBOUNDED || st == TR_CAPPED;
    const bool thin = st == TR_OPTIMAL && !(S.x[nt] > tol);
    const double px = lane < nt ? S.x[lane] : 0.0;
    if (thin) {
        if (lane < RD_WORDS) {
            const int left = m - 64 * lane;
            s_kept[lane] = left >= 64 ? ~0ull : left > 0 ? (1ull << left) - 1ull : 0ull;
        }
    } else {
        rd_row_loop<false>(S, m, nt, tol, px, pivots, lps, wide, s_kept);
    }
    __syncthreads();
    if (lane < RD_WORDS) a.kept[q * RD_WORDS + lane] = s_kept[lane];
    if (a.point && lane < nt) a.point[q * nt + lane] = px;
    if (lane == 0) {
        a.status[q] = thin ? RD_THIN : RD_OK;
        a.wide[q] = (int32_t)wide;
        atomicAdd(a.counters + 0, 1ull);
        atomicAdd(a.counters + 1, thin ? 1ull : 0ull);
        atomicAdd(a.counters + 2, lps);
        atomicAdd(a.counters + 3, pivots);
        atomicAdd(a.counters + 4, wide);
    }
}

}  // namespace mpc
