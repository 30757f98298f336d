// overlap.hpp -- the LPs of Solution.remove_overlaps (gfx950): the pair stage and the region difference; DESIGN §3.19.
//
// Regions and pieces arrive as unit rows [o | n] (|n| = 1, polytope {theta : n.theta <= o}), at most OV_MAX_ROWS each.  Every LP is a
// run of the wavefront vertex simplex of simplex.hpp over rows in LDS; one WAVEFRONT (workgroup of 64) per item.
//
//   radius run      max t  s.t.  n_r.theta + t <= o_r for every row: the Chebyshev radius.  Column n_t of a row is 1; the run starts
//                   from ANY theta with t = the smallest slack there (feasible, t may be negative), so it needs no phase 1.
//   k_overlap_pairs one wavefront per candidate pair (i, j): the rows of R_i and R_j together, the full radius r of the intersection
//                   and, when r > tol and the pair has a cut row [o | n] (the unit row of {J_j <= J_i}), d_min and d_max over the
//                   intersection of the depth d(theta) = o - n.theta = (J_i - J_j) / |g| behind the cut plane, from the Chebyshev
//                   centre with a warm start between the two.  flag[pair] = 1: a run was unbounded or stopped at the pivot cap.
//   k_overlap_split one wavefront per (piece P, cutter C): C = the rows of a region, then the item's cut row if it has one.  LDS rows
//                   [0, m_P): P; [m_P, m_P + m_C): the region's rows; m_P + m_C: the cut row.
//     intersection  radius(P n C), the run stops once t > tol.  Not above tol: P stays (flag bit 0 clear, empty mask).
//     row loop      ov_difference, the one loop of the two difference kernels (k_exit_split of exit_sets.hpp is the other), in place.
//                   Row k of the cutter is read from its own slot m_P + k (a slot with flag 2, a row k_exit_split dropped, is skipped)
//                   and written reversed into slot m_P + n_cut, n_cut the number of rows that have cut so far.  P n {earlier cutting
//                   rows} n {n_k.theta >= o_k} has radius > tol (the run stops there) iff row k cuts; the row is then turned forward
//                   in that slot and bounds every later candidate.  A run that is unbounded or capped counts as "cuts" (an empty
//                   child is found empty later; a dropped one would lose area).
//                   The slots hold the bits of the rows in global memory: ov_load stored exactly row[1 + t] and row[0], and
//                   tr_simplex writes neither A nor b.  n_cut <= k, so slot m_P + n_cut never lies behind slot m_P + k: the rows
//                   still to be read are untouched.  k_overlap_split has no flag 2 rows.
//     output        ov_finish.  flag[item]: bit 0 P meets C, bit 1 the cut row cuts, bit 2 some run was unbounded or capped;
//                   mask[item][OV_WORDS]: bit k, row k of the cutter's region cuts.  The host assembles the child pieces from these alone.
//   The only atomics are the counters; no floating-point atomics: a rerun gives the same bits.
#pragma once
#include <stdint.h>

#include "simplex.hpp"

namespace mpc {

constexpr int OV_MAX_ROWS = 256, OV_WORDS = OV_MAX_ROWS / 64;

// rows [r0, r0 + m) of a table of unit rows [o | n] into the LDS rows [at, at + m), as n.theta + t <= o
__device__ inline void ov_load(const TrLds &S, const double *ef, long long r0, int m, int nt, int at) {
    const int lane = threadIdx.x & 63, nr = nt + 1;
    for (int i = lane; i < m; i += 64) {
        const double *row = ef + (r0 + i) * (long long)nr;
        for (int t = 0; t < nt; ++t) S.A[(at + i) * nr + t] = row[1 + t];
        S.A[(at + i) * nr + nt] = 1.0;
        S.b[at + i] = row[0];
        S.flag[at + i] = 0;
    }
}

// the radius run over the LDS rows [0, m) from theta = S.x[0 .. nt): ends with the status of tr_simplex and t in S.x[nt]
__device__ inline int ov_radius(const TrLds &S, int m, int nt, double stop_t, unsigned long long &pivots) {
    const int lane = threadIdx.x & 63, nr = nt + 1;
    __syncthreads();
    double t0 = INFINITY;
    for (int r = lane; r < m; r += 64) {
        double s = S.b[r];
        for (int i = 0; i < nt; ++i) s = fma(-S.A[r * nr + i], S.x[i], s);
        t0 = fmin(t0, s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t0 = fmin(t0, __shfl_xor(t0, off));
    if (lane < TR_D) {
        if (lane >= nt) S.x[lane] = lane == nt ? t0 : 0.0;
        S.c[lane] = lane == nt ? -1.0 : 0.0;
    }
    tr_reset_basis(S, m, nt + 1);
    const int st = tr_simplex(S, m, nt, nt + 1, false, pivots, stop_t);
    __syncthreads();
    return st;
}

// The row loop of a region difference (the header comment): the candidates are the LDS rows [m_p, m_p + n_rows) behind the piece's rows
// [0, m_p); mask bit k is set for a cutting row k < n_mask.  Returns whether a row k >= n_mask cut.  s_mask is zeroed by the caller.
__device__ inline bool ov_difference(const TrLds &S, int m_p, int n_rows, int n_mask, int nt, double tol, unsigned long long &pivots,
                                     unsigned long long &lps, unsigned long long &wide, unsigned long long *s_mask) {
    const int lane = threadIdx.x & 63, nr = nt + 1;
    int n_cut = 0;
    bool tail_cuts = false;
    for (int k = 0; k < n_rows; ++k) {
        const int src = m_p + k, at = m_p + n_cut;
        __syncthreads();
        if (S.flag[src] == 2) continue;
        const double v = lane < nt ? S.A[src * nr + lane] : 0.0, rhs = S.b[src];
        __syncthreads();
        if (lane < nt) S.A[at * nr + lane] = -v;
        if (lane == 0) { S.A[at * nr + nt] = 1.0; S.b[at] = -rhs; S.flag[at] = 0; }
        const int st = ov_radius(S, at + 1, nt, tol, pivots);
        ++lps;
        wide += st == TR_UNBOUNDED || st == TR_CAPPED;
        if (st == TR_OPTIMAL && !(S.x[nt] > tol)) continue;
        // row k cuts: it bounds every later candidate
        __syncthreads();
        if (lane < nt) S.A[at * nr + lane] = v;
        if (lane == 0) {
            S.b[at] = rhs;
            if (k < n_mask) s_mask[k >> 6] |= 1ull << (k & 63);
        }
        if (k >= n_mask) tail_cuts = true;
        ++n_cut;
    }
    return tail_cuts;
}

// what an item of a difference kernel leaves: its flag bits, its mask from s_mask, and the counters items, meets, LPs, pivots, wide
__device__ inline void ov_finish(long long q, bool meets, bool cut_row_cuts, unsigned long long lps, unsigned long long pivots,
                                 unsigned long long wide, const unsigned long long *s_mask, int32_t *flag, unsigned long long *mask,
                                 unsigned long long *counters) {
    const int lane = threadIdx.x & 63;
    __syncthreads();
    if (lane < OV_WORDS) mask[q * OV_WORDS + lane] = s_mask[lane];
    if (lane == 0) {
        flag[q] = (meets ? 1 : 0) | (cut_row_cuts ? 2 : 0) | (wide ? 4 : 0);
        atomicAdd(counters + 0, 1ull);
        atomicAdd(counters + 1, meets ? 1ull : 0ull);
        atomicAdd(counters + 2, lps);
        atomicAdd(counters + 3, pivots);
        atomicAdd(counters + 4, wide);
    }
}

struct OverlapPairArgs {
    int nt, m_max;                   // m_max: LDS rows, at least m_i + m_j of every pair
    long long n_pairs;
    const long long *row_off;
    const double *ef;                // [rows][nt + 1] unit [o | n]
    const double *xs;                // [n_regions][nt] where the radius run of a pair starts (region i's row); any finite point
    const int32_t *pair_a, *pair_b, *has_cut;
    const double *cut;               // [n_pairs][nt + 1] unit cut rows, read where has_cut
    double tol;
    double *radius, *d_min, *d_max;  // d_min, d_max: NaN where not computed
    int32_t *flag;
    unsigned long long *counters;    // pairs, LPs, pivots, capped
};

__global__ void __launch_bounds__(64) k_overlap_pairs(OverlapPairArgs a) {
    extern __shared__ double ov_smem[];
    const int lane = threadIdx.x & 63, nt = a.nt, nr = nt + 1;
    const long long q = blockIdx.x;
    if (q >= a.n_pairs) return;
    const TrLds S = tr_lds(ov_smem, a.m_max, nt);
    const long long reg_i = a.pair_a[q], reg_j = a.pair_b[q], r0_i = a.row_off[reg_i], r0_j = a.row_off[reg_j];
    const int m_i = (int)(a.row_off[reg_i + 1] - r0_i), m_j = (int)(a.row_off[reg_j + 1] - r0_j), m = m_i + m_j;
    unsigned long long pivots = 0, capped = 0, lps = 1;
    ov_load(S, a.ef, r0_i, m_i, nt, 0);
    ov_load(S, a.ef, r0_j, m_j, nt, m_i);
    if (lane < TR_D) S.x[lane] = lane < nt ? a.xs[reg_i * nt + lane] : 0.0;
    const int st = ov_radius(S, m, nt, INFINITY, pivots);
    const double r = S.x[nt];
    int flag = st != TR_OPTIMAL;
    capped += st == TR_CAPPED;
    double dmin = NAN, dmax = NAN;
    if (!flag && r > a.tol && a.has_cut[q]) {
        // from the Chebyshev centre, in theta alone; the second run starts at the optimum of the first
        const double *row = a.cut + q * nr;
        tr_reset_basis(S, m, nt);
        const double lo = tr_min_plane(S, row + 1, 1.0, m, nt, pivots, capped);      // min n.theta, -inf when unbounded or capped
        const double hi = -tr_min_plane(S, row + 1, -1.0, m, nt, pivots, capped);    // max n.theta, +inf
        lps += 2;
        dmin = row[0] - hi;
        dmax = row[0] - lo;
        if (isinf(lo) || isinf(hi)) flag = 1;
    }
    if (lane == 0) {
        a.radius[q] = r;
        a.d_min[q] = dmin;
        a.d_max[q] = dmax;
        a.flag[q] = flag;
        atomicAdd(a.counters + 0, 1ull);
        atomicAdd(a.counters + 1, lps);
        atomicAdd(a.counters + 2, pivots);
        atomicAdd(a.counters + 3, capped);
    }
}

struct OverlapSplitArgs {
    int nt, m_max;                        // m_max: LDS rows, at least m_P + m_C + 2 of every item
    long long n_items;
    const long long *row_off, *piece_off;
    const double *ef, *piece_ef;          // the regions (cutters) and the pieces, unit [o | n]
    const int32_t *item_piece, *item_cutter, *has_cut;
    const double *cut;                    // [n_items][nt + 1], read where has_cut
    const double *start;                  // [n_items][nt] where the first run starts, or nullptr: the origin
    double tol;
    int32_t *flag;
    unsigned long long *mask;             // [n_items][OV_WORDS]
    unsigned long long *counters;         // items, items whose piece meets the cutter, LPs, pivots, unbounded or capped runs
};

__global__ void __launch_bounds__(64) k_overlap_split(OverlapSplitArgs a) {
    extern __shared__ double ov_smem[];
    __shared__ unsigned long long s_mask[OV_WORDS];
    const int lane = threadIdx.x & 63, nt = a.nt;
    const long long q = blockIdx.x;
    if (q >= a.n_items) return;
    const TrLds S = tr_lds(ov_smem, a.m_max, nt);
    const long long pc = a.item_piece[q], reg = a.item_cutter[q], p0 = a.piece_off[pc], c0 = a.row_off[reg];
    const int m_p = (int)(a.piece_off[pc + 1] - p0), m_c = (int)(a.row_off[reg + 1] - c0), hc = a.has_cut[q] ? 1 : 0, p = m_c + hc;
    const double tol = a.tol;
    unsigned long long pivots = 0, wide = 0, lps = 1;
    ov_load(S, a.piece_ef, p0, m_p, nt, 0);
    ov_load(S, a.ef, c0, m_c, nt, m_p);
    if (hc) ov_load(S, a.cut, q, 1, nt, m_p + m_c);
    if (lane < TR_D) S.x[lane] = (lane < nt && a.start) ? a.start[q * nt + lane] : 0.0;
    if (lane < OV_WORDS) s_mask[lane] = 0ull;
    int st = ov_radius(S, m_p + p, nt, tol, pivots);
    wide += st == TR_UNBOUNDED || st == TR_CAPPED;
    const bool meets = !(st == TR_OPTIMAL && !(S.x[nt] > tol));
    const bool cut_row_cuts = meets && ov_difference(S, m_p, p, m_c, nt, tol, pivots, lps, wide, s_mask);
    ov_finish(q, meets, cut_row_cuts, lps, pivots, wide, s_mask, a.flag, a.mask, a.counters);
}

}  // namespace mpc
