// exit_sets.hpp -- the LPs of Solution.exit_sets (gfx950): the region difference against a pulled-back cutter; DESIGN §3.21.
//
// Regions and pieces arrive as unit rows [o | n] (|n| = 1, polytope {theta : n.theta <= o}), at most OV_MAX_ROWS each; region i carries
// the closed-loop map theta+ = Phi_i theta + phi_i.  The cutter of an item (piece P of source region i, target region j) is
// C_ij = {theta : Phi_i theta + phi_i in R_j}: the rows of R_j pulled back through the map of i by ts_pull_back (transition.hpp), the
// arithmetic of k_transition_pairs.  Every LP is a radius run (ov_radius, overlap.hpp) over rows in LDS; one WAVEFRONT (workgroup of 64)
// per item.
//
//   k_exit_split  LDS rows [0, m_P): P; [m_P, m_P + m_j): the pulled-back rows, a constant one as flag 2 with right-hand side +inf.
//     empty cutter  a constant row with beta < -tol: C_ij is empty, P stays (flag 0, empty mask), no LP.
//     intersection  radius(P n C), the run stops once t > tol.  Not above tol: P stays.
//     row loop      ov_difference (overlap.hpp), the one loop of the two difference kernels, in place over the slots [m_P, m_P + m_j):
//                   dropped rows (flag 2) are skipped, every row of the target region has a mask bit.
//     output        flag[item]: bit 0 P meets C, bit 2 some run was unbounded or capped (the bits of k_overlap_split; bit 1 is never set);
//                   mask[item][OV_WORDS]: bit k, row k of the target region cuts.  The host assembles the child pieces from these alone.
//   The only atomics are the counters; no floating-point atomics: a rerun gives the same bits.
#pragma once
#include <stdint.h>

#include "transition.hpp"

namespace mpc {

struct ExitSplitArgs {
    int nt, m_max;                        // m_max: LDS rows, at least m_P + m_j of every item
    long long n_items;
    const long long *row_off, *piece_off;
    const double *ef, *piece_ef;          // the regions and the pieces, unit [o | n]
    const double *Phi, *phi;              // [n_regions][nt][nt], [n_regions][nt]
    const int32_t *item_piece, *item_source, *item_target;
    const double *start;                  // [n_items][nt] where the first run starts, or nullptr: the origin
    double tol;
    int32_t *flag;
    unsigned long long *mask;             // [n_items][OV_WORDS]
    unsigned long long *counters;         // items, items whose piece meets the cutter, LPs, pivots, unbounded or capped runs
};

__global__ void __launch_bounds__(64) k_exit_split(ExitSplitArgs a) {
    extern __shared__ double ex_smem[];
    __shared__ unsigned long long s_mask[OV_WORDS];
    const int lane = threadIdx.x & 63, nt = a.nt;
    const long long q = blockIdx.x;
    if (q >= a.n_items) return;
    const TrLds S = tr_lds(ex_smem, a.m_max, nt);
    const long long pc = a.item_piece[q], reg_i = a.item_source[q], reg_j = a.item_target[q], p0 = a.piece_off[pc], c0 = a.row_off[reg_j];
    const int m_p = (int)(a.piece_off[pc + 1] - p0), m_c = (int)(a.row_off[reg_j + 1] - c0);
    const double tol = a.tol;
    unsigned long long pivots = 0, wide = 0, lps = 0;
    ov_load(S, a.piece_ef, p0, m_p, nt, 0);
    const int empty = ts_pull_back(S, a.ef, c0, m_c, nt, m_p, a.Phi + reg_i * (long long)nt * nt, a.phi + reg_i * nt, tol);
    if (lane < TR_D) S.x[lane] = (lane < nt && a.start) ? a.start[q * nt + lane] : 0.0;
    if (lane < OV_WORDS) s_mask[lane] = 0ull;
    bool meets = false;
    if (!__any(empty)) {
        int st = ov_radius(S, m_p + m_c, nt, tol, pivots);
        lps = 1;
        wide += st == TR_UNBOUNDED || st == TR_CAPPED;
        meets = !(st == TR_OPTIMAL && !(S.x[nt] > tol));
    }
    if (meets) ov_difference(S, m_p, m_c, m_c, nt, tol, pivots, lps, wide, s_mask);
    ov_finish(q, meets, false, lps, pivots, wide, s_mask, a.flag, a.mask, a.counters);
}

}  // namespace mpc
