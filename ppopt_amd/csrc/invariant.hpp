// invariant.hpp -- the LPs of Solution.invariant_set (gfx950): the backward exit cells of a closed loop; DESIGN §3.23.
//
// Regions and cells arrive as unit rows [o | n] (|n| = 1, polytope {theta : n.theta <= o}), at most OV_MAX_ROWS each; region i carries
// the closed-loop map theta+ = Phi_i theta + phi_i.  A cell Q of step k holds states that leave the solution after exactly k + 1 steps;
// an item (region i, cell Q) asks for R_i n f_i^-1(Q), a cell of step k + 1.  Every LP is a radius run (ov_radius, overlap.hpp) over rows
// in LDS; one WAVEFRONT (workgroup of 64) per item.  The cells of all steps live in one CSR table on the device, which the kernels read
// (the parents) and write (the children): their rows never visit the host between steps.
//
//   k_pre_cells  LDS rows [0, m_i): R_i; [m_i, m_i + m_Q): the rows of Q pulled back through the map of i by ts_pull_back (transition.hpp),
//                a constant one as flag 2 with right-hand side +inf.
//     empty        a constant row with beta < -tol: no state of R_i lands in Q (PC_EMPTY), no LP.
//     radius run   over the m_i + m_Q rows from region i's feasible point, the run stops once t > tol.  Optimal with t <= tol: PC_NONE.
//                  Otherwise the item is a cell: PC_CELL, or PC_CELL_WIDE behind an unbounded or capped run, when the cell may hold
//                  states that stay.
//     row loop     rd_row_loop (reduce.hpp), the one loop of k_reduce_rows, in place over all slots in order: the region's rows, then
//                  the pulled-back ones; dropped slots are skipped; every run starts where the radius run ended.  An unbounded or capped run
//                  keeps its row, which changes no set; like the radius run it counts in counters[5].
//     output       status[item], kept[item][RD_WORDS] (bit k: slot k stays), n_kept[item], point[item][n_t] (where the radius run ended).
//   k_pre_emit   one wavefront per cell: the same ov_load and ts_pull_back, so the slots hold bit for bit the rows that were judged; the
//                kept slots go to the rows [cell_off[c], cell_off[c] + n_kept) of the cell table in slot order.  No LP.
//   The only atomics are the counters; no floating-point atomics: a rerun gives the same bits.
//
// What the forward cells (forward.hpp) do the same way is here once, and knows nothing of its caller: pc_judge, everything
// of a cell kernel from the radius run to the counters, and pc_scatter, the stores of an emit kernel into the cell table.  What differs
// (which rows are loaded and which pulled back, through which map, from which start point) is the four kernels.
#pragma once
#include <stdint.h>

#include "reduce.hpp"
#include "transition.hpp"

namespace mpc {

enum { PC_NONE = 0, PC_CELL = 1, PC_EMPTY = 2, PC_CELL_WIDE = 3 };

// The judging tail of item q of a cell kernel.  The caller has put the item's m rows into the slots of S, its start point into S.x,
// zeroes into s_kept [RD_WORDS] of LDS, and passes ``empty`` (wavefront-uniform) of its ts_pull_back.  The radius run, the row loop, then
// status[q], kept[q][RD_WORDS], n_kept[q], point[q][nt] and the six counters.
__device__ inline void pc_judge(const TrLds &S, int m, int nt, double tol, int empty, unsigned long long *s_kept, long long q, int32_t *status,
                                int32_t *n_kept, unsigned long long *kept, double *point, unsigned long long *counters) {
    const int lane = threadIdx.x & 63;
    unsigned long long pivots = 0, wide = 0, lps = 0;
    bool is_cell = false, open = false;
    double px = 0.0;
    if (!empty) {
        const int st = ov_radius(S, m, nt, tol, pivots);
        lps = 1;
        open = st == TR_UNBOUNDED || st == TR_CAPPED;
        wide += open;
        is_cell = !(st == TR_OPTIMAL && !(S.x[nt] > tol));
        px = lane < nt ? S.x[lane] : 0.0;
    }
    if (is_cell) rd_row_loop<true>(S, m, nt, tol, px, pivots, lps, wide, s_kept);
    __syncthreads();
    int count = 0;
    if (lane < RD_WORDS) {
        kept[q * RD_WORDS + lane] = s_kept[lane];
        count = __popcll(s_kept[lane]);
    }
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) count += __shfl_xor(count, off);
    if (lane < nt) point[q * nt + lane] = px;
    if (lane == 0) {
        status[q] = empty ? PC_EMPTY : !is_cell ? PC_NONE : open ? PC_CELL_WIDE : PC_CELL;
        n_kept[q] = count;
        atomicAdd(counters + 0, 1ull);
        atomicAdd(counters + 1, is_cell ? 1ull : 0ull);
        atomicAdd(counters + 2, empty ? 1ull : 0ull);
        atomicAdd(counters + 3, lps);
        atomicAdd(counters + 4, pivots);
        atomicAdd(counters + 5, wide);
    }
}

// The slots k of S (0 .. m) with bit k of mask [RD_WORDS] set, to the rows [out0, out1) of the cell table in slot order.
__device__ inline void pc_scatter(const TrLds &S, int m, int nt, const unsigned long long *mask, long long out0, long long out1, double *cell_ef) {
    const int lane = threadIdx.x & 63, nr = nt + 1;
    for (int k = lane; k < m; k += 64) {
        const int w = k >> 6;
        const unsigned long long word = mask[w];
        if (!((word >> (k & 63)) & 1ull)) continue;
        long long at = out0 + __popcll(word & ((1ull << (k & 63)) - 1ull));
        for (int u = 0; u < w; ++u) at += __popcll(mask[u]);
        if (at >= out1) continue;         // the scan and the mask agree by construction: never taken, and never a store past the cell
        double *out = cell_ef + at * (long long)nr;
        out[0] = S.b[k];
        for (int t = 0; t < nt; ++t) out[1 + t] = S.A[k * nr + t];
    }
}

struct PreCellArgs {
    int nt, m_max;                        // m_max: LDS rows, at least m_i + m_Q of every item
    long long n_items;
    const long long *row_off, *cell_off;
    const double *ef, *cell_ef;           // the regions and the cell table, unit [o | n]
    const double *Phi, *phi, *xs;         // [n_regions][nt][nt], [n_regions][nt], [n_regions][nt] a feasible point of every region
    const int32_t *item_region, *item_cell;
    double tol;
    int32_t *status, *n_kept;
    unsigned long long *kept;             // [n_items][RD_WORDS]
    double *point;                        // [n_items][nt]
    unsigned long long *counters;         // items, cells, items emptied by a constant row, LPs, pivots, unbounded or capped runs
};

__global__ void __launch_bounds__(64) k_pre_cells(PreCellArgs a) {
    extern __shared__ double pc_smem[];
    __shared__ unsigned long long s_kept[RD_WORDS];
    const int lane = threadIdx.x & 63, nt = a.nt;
    const long long q = blockIdx.x;
    if (q >= a.n_items) return;
    const TrLds S = tr_lds(pc_smem, a.m_max, nt);
    const long long reg = a.item_region[q], cell = a.item_cell[q], r0 = a.row_off[reg], c0 = a.cell_off[cell];
    const int m_i = (int)(a.row_off[reg + 1] - r0), m_q = (int)(a.cell_off[cell + 1] - c0), m = m_i + m_q;
    const double tol = a.tol;
    ov_load(S, a.ef, r0, m_i, nt, 0);
    const int empty = __any(ts_pull_back(S, a.cell_ef, c0, m_q, nt, m_i, a.Phi + reg * (long long)nt * nt, a.phi + reg * nt, tol));
    if (lane < TR_D) S.x[lane] = lane < nt ? a.xs[reg * nt + lane] : 0.0;
    if (lane < RD_WORDS) s_kept[lane] = 0ull;
    pc_judge(S, m, nt, tol, empty, s_kept, q, a.status, a.n_kept, a.kept, a.point, a.counters);
}

struct PreEmitArgs {
    int nt, m_max;
    long long n_cells;                    // the new cells: cell c of this launch is cell first_cell + c of the table
    long long first_cell;
    const long long *row_off;
    const long long *cell_off;            // of the parents and of the new cells (the host's scan of n_kept)
    const double *ef;
    double *cell_ef;                      // parents are read, the new cells' rows written: disjoint ranges of one table
    const double *Phi, *phi;
    const int32_t *item_region, *item_cell;
    const int32_t *cell_item;             // [n_cells] the item a new cell came from
    const unsigned long long *kept;       // [n_items][RD_WORDS] of k_pre_cells
    const double *point;                  // [n_items][nt] of k_pre_cells
    double *cell_point;                   // [cells][nt]
    double tol;
};

__global__ void __launch_bounds__(64) k_pre_emit(PreEmitArgs a) {
    extern __shared__ double pc_smem[];
    const int lane = threadIdx.x & 63, nt = a.nt;
    const long long c = blockIdx.x;
    if (c >= a.n_cells) return;
    const TrLds S = tr_lds(pc_smem, a.m_max, nt);
    const long long q = a.cell_item[c], reg = a.item_region[q], cell = a.item_cell[q], r0 = a.row_off[reg], c0 = a.cell_off[cell];
    const int m_i = (int)(a.row_off[reg + 1] - r0), m_q = (int)(a.cell_off[cell + 1] - c0), m = m_i + m_q;
    const long long out0 = a.cell_off[a.first_cell + c], out1 = a.cell_off[a.first_cell + c + 1];
    ov_load(S, a.ef, r0, m_i, nt, 0);
    (void)ts_pull_back(S, a.cell_ef, c0, m_q, nt, m_i, a.Phi + reg * (long long)nt * nt, a.phi + reg * nt, a.tol);
    __syncthreads();
    if (lane < nt) a.cell_point[(a.first_cell + c) * nt + lane] = a.point[q * nt + lane];
    pc_scatter(S, m, nt, a.kept + q * RD_WORDS, out0, out1, a.cell_ef);
}

}  // namespace mpc
