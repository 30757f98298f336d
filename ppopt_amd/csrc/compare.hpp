// compare.hpp -- the LPs of Solution.compare (gfx950): the largest gap between two affine laws over the intersection of two regions;
// DESIGN §3.26.
//
// Regions arrive as unit rows [o | n] (|n| = 1, polytope {theta : n.theta <= o}), at most OV_MAX_ROWS each, in ONE table that holds the
// regions of both solutions; laws as [n_regions][n_out][n_t + 1] = [b | A].  Every LP is a run of the wavefront vertex simplex of
// simplex.hpp over rows in LDS; one WAVEFRONT (workgroup of 64) per pair, as in k_overlap_pairs (overlap.hpp), the model of this kernel.
//
//   k_law_gap     pair (i, j): the rows of R_i and R_j together (ov_load), the full radius r of X = R_i n R_j from xs[i] (ov_radius).
//     r <= tol    the pair does not meet: gap NaN, row -1, witness and range NaN.  Facet neighbours and disjoint regions end here.
//     open radius the run was unbounded (radius +inf) or stopped at the pivot cap (radius: the value reached): gap +inf, row -1, flag 1,
//                 witness the point reached, range NaN, no law LP.
//     r > tol     for every output row k in order, delta_k(theta) = (A_i[k] - A_j[k]).theta + (b_i[k] - b_j[k]):
//                   A_i[k] == A_j[k] in every entry (compared as doubles, no threshold): the row is constant, lo = hi = b_i[k] - b_j[k],
//                   no LP; a gap it gives has the Chebyshev centre as its witness;
//                   otherwise lo = min delta_k, then hi = max delta_k over X by tr_min_plane, each run warm-started where the previous
//                   one ended (the first from the Chebyshev centre after tr_reset_basis).  An unbounded or capped run gives lo = -inf or
//                   hi = +inf, hence gap +inf and flag 1: a bound, not a value.
//                 gap = max_k max(-lo_k, hi_k); the candidates are taken in the order row 0 min, row 0 max, row 1 min, ... and a later one
//                 replaces an earlier one only when strictly larger, so row is the lowest k that attains the gap and witness the theta
//                 where that run ended.
//   The only atomics are the counters; no floating-point atomics: a rerun gives the same bits.
#pragma once
#include <stdint.h>

#include "overlap.hpp"

namespace mpc {

constexpr int LG_MAX_OUT = 256;

struct LawGapArgs {
    int nt, m_max, n_out;            // m_max: LDS rows, at least m_i + m_j of every pair
    long long n_pairs;
    const long long *row_off;
    const double *ef;                // [rows][nt + 1] unit [o | n]
    const double *laws;              // [n_regions][n_out][nt + 1] = [b | A]
    const double *xs;                // [n_regions][nt] where the radius run of a pair starts (region i's row); any finite point
    const int32_t *pair_a, *pair_b;
    double tol;
    double *radius, *gap, *witness;  // witness [n_pairs][nt]
    double *range;                   // [n_pairs][n_out][2] = lo, hi, or nullptr
    int32_t *gap_row, *flag;
    unsigned long long *counters;    // pairs, pairs that meet, constant rows, LPs, pivots, unbounded or capped runs
};

__global__ void __launch_bounds__(64) k_law_gap(LawGapArgs a) {
    extern __shared__ double lg_smem[];
    __shared__ double s_d[TR_D], s_wit[TR_D], s_centre[TR_D];   // the row's normal difference, the witness so far, the Chebyshev centre
    const int lane = threadIdx.x & 63, nt = a.nt, nr = nt + 1, K = a.n_out;
    const long long q = blockIdx.x;
    if (q >= a.n_pairs) return;
    const TrLds S = tr_lds(lg_smem, a.m_max, nt);
    const long long reg_i = a.pair_a[q], reg_j = a.pair_b[q], r0_i = a.row_off[reg_i], r0_j = a.row_off[reg_j];
    const int m_i = (int)(a.row_off[reg_i + 1] - r0_i), m_j = (int)(a.row_off[reg_j + 1] - r0_j), m = m_i + m_j;
    unsigned long long pivots = 0, capped = 0, wide = 0, lps = 1, constant = 0;
    ov_load(S, a.ef, r0_i, m_i, nt, 0);
    ov_load(S, a.ef, r0_j, m_j, nt, m_i);
    if (lane < TR_D) S.x[lane] = lane < nt ? a.xs[reg_i * nt + lane] : 0.0;
    const int st = ov_radius(S, m, nt, INFINITY, pivots);
    const double r = st == TR_UNBOUNDED ? INFINITY : S.x[nt];
    int flag = st != TR_OPTIMAL, row = -1;
    wide += flag;
    const bool meets = !flag && r > a.tol;
    double gap = flag ? INFINITY : NAN;
    if (lane < nt) s_wit[lane] = (flag || meets) ? S.x[lane] : NAN;
    if (a.range && !meets)
        for (int k = lane; k < 2 * K; k += 64) a.range[q * 2 * K + k] = NAN;
    if (meets) {
        // from the Chebyshev centre, in theta alone; every run starts at the optimum of the one before
        if (lane < nt) s_centre[lane] = S.x[lane];
        tr_reset_basis(S, m, nt);
        gap = -INFINITY;
        for (int k = 0; k < K; ++k) {
            const double *li = a.laws + (reg_i * K + k) * nr, *lj = a.laws + (reg_j * K + k) * nr;
            const double vi = lane < nt ? li[1 + lane] : 0.0, vj = lane < nt ? lj[1 + lane] : 0.0, c0 = li[0] - lj[0];
            double lo = c0, hi = c0;
            if (!__any(vi != vj)) {
                ++constant;
                if (fabs(c0) > gap) {
                    gap = fabs(c0);
                    row = k;
                    if (lane < nt) s_wit[lane] = s_centre[lane];
                }
            } else {
                __syncthreads();
                if (lane < TR_D) s_d[lane] = vi - vj;
                lo = tr_min_plane(S, s_d, 1.0, m, nt, pivots, capped) + c0;      // min delta_k, -inf when unbounded or capped
                if (-lo > gap) {
                    gap = -lo;
                    row = k;
                    if (lane < nt) s_wit[lane] = S.x[lane];
                }
                hi = -tr_min_plane(S, s_d, -1.0, m, nt, pivots, capped) + c0;    // max delta_k, +inf
                if (hi > gap) {
                    gap = hi;
                    row = k;
                    if (lane < nt) s_wit[lane] = S.x[lane];
                }
                lps += 2;
                wide += (isinf(lo) ? 1 : 0) + (isinf(hi) ? 1 : 0);
                if (isinf(lo) || isinf(hi)) flag = 1;
            }
            if (a.range && lane == 0) {
                a.range[(q * K + k) * 2] = lo;
                a.range[(q * K + k) * 2 + 1] = hi;
            }
        }
        gap = fabs(gap);     // hi_k >= lo_k, so gap >= 0: only a -0.0 (from a minimum of +0.0) changes
    }
    __syncthreads();
    if (lane < nt) a.witness[q * nt + lane] = s_wit[lane];
    if (lane == 0) {
        a.radius[q] = r;
        a.gap[q] = gap;
        a.gap_row[q] = row;
        a.flag[q] = flag;
        atomicAdd(a.counters + 0, 1ull);
        atomicAdd(a.counters + 1, meets ? 1ull : 0ull);
        atomicAdd(a.counters + 2, constant);
        atomicAdd(a.counters + 3, lps);
        atomicAdd(a.counters + 4, pivots);
        atomicAdd(a.counters + 5, wide);
    }
}

}  // namespace mpc
