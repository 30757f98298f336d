// forward.hpp -- the LPs of Solution.reach_cells (gfx950): the forward cells of a closed loop in initial-state coordinates; DESIGN §3.25.
//
// Regions and cells arrive as unit rows [o | n] (|n| = 1, polytope {theta : n.theta <= o}), at most OV_MAX_ROWS each; region i carries
// the closed-loop map theta+ = Phi_i theta + phi_i.  A cell Q of step k is a set of INITIAL states theta_0: the ones whose state at step
// k lies in region(Q), with theta_k = G theta_0 + g on Q.  An item (cell Q, region j), j a successor of region(Q), asks for
// Q n {theta_0 : P theta_0 + s in R_j}, a cell of step k + 1, with the NEXT MAP of Q: P = Phi_i G, s = Phi_i g + phi_i, i = region(Q).
// A map is pulled back through and never inverted.  Every LP is a radius run (ov_radius, overlap.hpp) over rows in LDS; one WAVEFRONT
// (workgroup of 64) per item.  The cells of all steps live in one CSR table on the device with their points and maps [n_t][n_t + 1] =
// [G | g], which the kernels read (the parents) and write (the children): rows and maps never visit the host between steps.
//
//   k_fwd_maps   one wavefront per cell of the last step: next[c] = [P | s], every entry one sum over t ascending from 0.0 of plain
//                products (the unit is compiled without contraction): a rerun and the reference's explicit loop give the same bits.
//   k_fwd_cells  LDS rows [0, m_Q): Q from the cell table (ov_load); [m_Q, m_Q + m_j): the rows of R_j pulled back through the next map
//                of Q by ts_pull_back (transition.hpp), a constant one as flag 2 with right-hand side +inf.  The map is staged in LDS as
//                [n_t][n_t] and [n_t], the layout ts_pull_back reads.
//     empty        a constant row with beta < -tol: no state of Q lands in R_j (PC_EMPTY), no LP.
//     the rest     pc_judge of invariant.hpp, the tail k_pre_cells runs: the radius run over the m_Q + m_j rows from Q's point, the row
//                  loop over all slots in order (Q's rows, then the pulled-back ones), status, kept, n_kept, point and the counters.
//   k_fwd_emit   one wavefront per new cell: the same ov_load and ts_pull_back, so the slots hold bit for bit the rows that were judged;
//                the kept slots go to the rows [cell_off[c], cell_off[c] + n_kept) of the cell table in slot order (pc_scatter of
//                invariant.hpp); the parent's next map becomes the child's [G | g], the item's point the child's point.  No LP.
//   The only atomics are the counters; no floating-point atomics: a rerun gives the same bits.
#pragma once
#include <stdint.h>

#include "invariant.hpp"

namespace mpc {

// next[c - first][r][0 .. nt) = sum_t Phi_i[r][t] G_c[t][.], next[..][r][nt] = sum_t Phi_i[r][t] g_c[t] + phi_i[r]
__global__ void __launch_bounds__(64) k_fwd_maps(int nt, long long n_cells, long long first, const int32_t *__restrict__ cell_region,
                                                 const double *__restrict__ Phi, const double *__restrict__ phi,
                                                 const double *__restrict__ cell_map, double *__restrict__ next) {
    const int lane = threadIdx.x & 63, nr = nt + 1;
    const long long c = blockIdx.x;
    if (c >= n_cells) return;
    const long long reg = cell_region[first + c];
    const double *F = Phi + reg * (long long)nt * nt, *M = cell_map + (first + c) * (long long)nt * nr;
    double *out = next + c * (long long)nt * nr;
    for (int e = lane; e < nt * nr; e += 64) {
        const int r = e / nr, k = e - r * nr;
        double acc = 0.0;
        for (int t = 0; t < nt; ++t) acc = acc + F[r * nt + t] * M[t * nr + k];
        if (k == nt) acc = acc + phi[reg * nt + r];
        out[e] = acc;
    }
}

// the map [nt][nt + 1] = [P | s] of global memory into P [nt][nt] and sh [nt] of LDS; the caller's next barrier publishes it
__device__ inline void fw_stage_map(const double *map, int nt, double *P, double *sh) {
    const int lane = threadIdx.x & 63, nr = nt + 1;
    for (int e = lane; e < nt * nr; e += 64) {
        const int r = e / nr, k = e - r * nr;
        if (k == nt) sh[r] = map[e];
        else P[r * nt + k] = map[e];
    }
}

struct FwdCellArgs {
    int nt, m_max;                        // m_max: LDS rows, at least m_Q + m_j of every item
    long long n_items;
    long long first;                      // the first cell of the last step: next[] is indexed by cell - first
    const long long *row_off, *cell_off;
    const double *ef, *cell_ef;           // the regions and the cell table, unit [o | n]
    const double *next;                   // [cells of the last step][nt][nt + 1] of k_fwd_maps
    const double *cell_point;             // [cells][nt]
    const int32_t *item_cell, *item_region;
    double tol;
    int32_t *status, *n_kept;
    unsigned long long *kept;             // [n_items][RD_WORDS]
    double *point;                        // [n_items][nt]
    unsigned long long *counters;         // items, cells, items emptied by a constant row, LPs, pivots, unbounded or capped runs
};

__global__ void __launch_bounds__(64) k_fwd_cells(FwdCellArgs a) {
    extern __shared__ double fw_smem[];
    __shared__ unsigned long long s_kept[RD_WORDS];
    __shared__ double s_P[TR_D * TR_D], s_sh[TR_D];
    const int lane = threadIdx.x & 63, nt = a.nt;
    const long long q = blockIdx.x;
    if (q >= a.n_items) return;
    const TrLds S = tr_lds(fw_smem, a.m_max, nt);
    const long long reg = a.item_region[q], cell = a.item_cell[q], r0 = a.row_off[reg], c0 = a.cell_off[cell];
    const int m_q = (int)(a.cell_off[cell + 1] - c0), m_j = (int)(a.row_off[reg + 1] - r0), m = m_q + m_j;
    const double tol = a.tol;
    fw_stage_map(a.next + (cell - a.first) * (long long)nt * (nt + 1), nt, s_P, s_sh);
    ov_load(S, a.cell_ef, c0, m_q, nt, 0);
    if (lane < TR_D) S.x[lane] = lane < nt ? a.cell_point[cell * nt + lane] : 0.0;
    if (lane < RD_WORDS) s_kept[lane] = 0ull;
    __syncthreads();
    const int empty = __any(ts_pull_back(S, a.ef, r0, m_j, nt, m_q, s_P, s_sh, tol));
    pc_judge(S, m, nt, tol, empty, s_kept, q, a.status, a.n_kept, a.kept, a.point, a.counters);
}

struct FwdEmitArgs {
    int nt, m_max;
    long long n_cells;                    // the new cells: cell c of this launch is cell first_cell + c of the table
    long long first_cell;
    long long first;                      // the first cell of the last step (next[] is indexed by parent - first)
    const long long *row_off;
    const long long *cell_off;            // of the parents and of the new cells (the host's scan of n_kept)
    const double *ef;
    double *cell_ef;                      // parents are read, the new cells' rows written: disjoint ranges of one table
    const double *next;
    double *cell_map;                     // [cells][nt][nt + 1]: the new cells' maps are written
    const int32_t *item_cell, *item_region;
    const int32_t *cell_item;             // [n_cells] the item a new cell came from
    const unsigned long long *kept;       // [n_items][RD_WORDS] of k_fwd_cells
    const double *point;                  // [n_items][nt] of k_fwd_cells
    double *cell_point;                   // [cells][nt]
    double tol;
};

__global__ void __launch_bounds__(64) k_fwd_emit(FwdEmitArgs a) {
    extern __shared__ double fw_smem[];
    __shared__ double s_P[TR_D * TR_D], s_sh[TR_D];
    const int lane = threadIdx.x & 63, nt = a.nt, nr = nt + 1;
    const long long c = blockIdx.x;
    if (c >= a.n_cells) return;
    const TrLds S = tr_lds(fw_smem, a.m_max, nt);
    const long long q = a.cell_item[c], reg = a.item_region[q], cell = a.item_cell[q], r0 = a.row_off[reg], c0 = a.cell_off[cell];
    const int m_q = (int)(a.cell_off[cell + 1] - c0), m_j = (int)(a.row_off[reg + 1] - r0), m = m_q + m_j;
    const long long out0 = a.cell_off[a.first_cell + c], out1 = a.cell_off[a.first_cell + c + 1];
    const double *map = a.next + (cell - a.first) * (long long)nt * nr;
    fw_stage_map(map, nt, s_P, s_sh);
    ov_load(S, a.cell_ef, c0, m_q, nt, 0);
    __syncthreads();
    (void)ts_pull_back(S, a.ef, r0, m_j, nt, m_q, s_P, s_sh, a.tol);
    __syncthreads();
    if (lane < nt) a.cell_point[(a.first_cell + c) * nt + lane] = a.point[q * nt + lane];
    for (int e = lane; e < nt * nr; e += 64) a.cell_map[(a.first_cell + c) * (long long)nt * nr + e] = map[e];
    pc_scatter(S, m, nt, a.kept + q * RD_WORDS, out0, out1, a.cell_ef);
}

}  // namespace mpc
