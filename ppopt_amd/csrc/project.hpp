// project.hpp -- projecting polytopes: Fourier-Motzkin elimination alternating with the row loop of reduce.hpp (gfx950); DESIGN §3.24.
//
// A polytope arrives as unit rows [o | n] (|n| = 1, {x : n.x <= o}), at most PJ_MAX_ROWS of them, in order; its trailing n_elim
// coordinates are eliminated one at a time, the last one first.  One WAVEFRONT (workgroup of 64) per polytope; every LP is a radius run
// (ov_radius, overlap.hpp) over rows in LDS.
//
//   LDS            two areas.  S: the TrLds of the runs, re-derived (tr_lds) for the dimension of every step.  R behind it: the live rows as
//                  raw [o | n] rows of stride d + 1, compacted, in order.  A step reads R and writes S, the reduce reads and writes S, the
//                  kept rows go back to R: the old rows never share an area with the new ones.  Both areas hold m_lds rows, the largest
//                  count any step of any item of the launch can reach (the host bounds it; PJ_MAX_ROWS with two steps or more).  R is in
//                  LDS and not in a global slab because the combinations read every old row |P| or |N| times from all lanes at once,
//                  and two areas still fit: 78,840 + 69,632 bytes at 512 rows and n = 16, plus 2,112 static.
//   thin test      radius(P) from the item's start point (the origin without one), the run stops once t > tol.  Optimal with t <= tol:
//                  PJ_THIN.  Otherwise lane i keeps x_i of the point where the run ended: the interior point.  With n_elim = 0 the row
//                  loop follows: one pass of k_reduce_rows.
//   step d -> d-1  c = a row's coefficient of coordinate j = d - 1; Z: |c| <= PJ_ZERO_COEF, P: c > PJ_ZERO_COEF, N: c < -PJ_ZERO_COEF.
//     classes      64 rows at a time: the rank of a row in its class is the bits of the ballot below its lane.  A row of Z goes
//                  straight to slot rank (bit for bit when c == 0, else scaled by the norm of what is left); P and N are index lists.
//     row limit    |Z| + |P||N| (|Z| when P or N is empty) > PJ_MAX_ROWS: PJ_TOO_LARGE.
//     combinations lane l takes the pairs l, l + 64, ...: pair i = p |N| + q, slot |Z| + i, the row (-c_q) row_p + c_p row_q without
//                  column j, scaled to a unit normal.  A normal of norm <= PJ_ZERO_NORM before scaling is the statement 0 <= rhs: the
//                  slot becomes a dropped row (flag 2, right-hand side +inf: it bounds no run and rd_row_loop<true> passes it over
//                  without an LP), and with rhs < -tol the item is PJ_THIN (empty).  No row left at all: PJ_WHOLE.
//     reduce       the interior point loses coordinate j; the thin test from it (PJ_THIN, or the point moves to where the run ended),
//                  then rd_row_loop over the slots.  The kept rows are compacted into R in order (the rank of a row is the number of
//                  kept bits below it) and are the live rows of the next step.
//   output         status[q]; n_out[q] and out_rows[q][out_cap][n - n_elim + 1] (PJ_OK only; more than out_cap rows: PJ_TOO_LARGE);
//                  wide[q]: the unbounded or capped runs (their rows were kept); peak[q]: the largest row count a step made;
//                  point[q][n - n_elim] (optional): the interior point in the kept coordinates (PJ_OK only).
//   The only atomics are the counters; no floating-point atomics: a rerun gives the same bits.
#pragma once
#include <stdint.h>

#include "reduce.hpp"

namespace mpc {

constexpr int PJ_MAX_ROWS = RD_MAX_ROWS;
constexpr double PJ_ZERO_COEF = 1e-12, PJ_ZERO_NORM = 1e-9;
enum { PJ_OK = 0, PJ_THIN = 1, PJ_WHOLE = 2, PJ_TOO_LARGE = 3 };

struct ProjectArgs {
    int n, n_elim, m_lds, out_cap;        // m_lds: rows of each LDS area
    long long n_poly;
    const long long *row_off;
    const double *ef;                     // unit [o | n]
    const double *start;                  // [n_poly][n] where the thin test starts, or nullptr: the origin
    double tol;
    int32_t *status, *n_out, *wide, *peak;
    double *out_rows;                     // [n_poly][out_cap][n - n_elim + 1]
    double *point;                        // [n_poly][n - n_elim], or nullptr
    unsigned long long *counters;         // items, thin, whole, too large, steps, rows made, LPs, pivots, unbounded or capped runs
};

// bytes of the TrLds area, a multiple of 8: the raw rows start behind it
__host__ __device__ inline size_t pj_s_bytes(int m_lds, int n) { return (tr_lds_bytes(m_lds, n) + 7) & ~(size_t)7; }
__host__ __device__ inline size_t pj_lds_bytes(int m_lds, int n) { return pj_s_bytes(m_lds, n) + (size_t)m_lds * (n + 1) * 8; }

// the raw rows R[0, m) of dimension d into the LDS rows of S, as n.x + t <= o
__device__ inline void pj_fill(const TrLds &S, const double *R, int m, int d) {
    const int lane = threadIdx.x & 63, nr = d + 1;
    for (int i = lane; i < m; i += 64) {
        for (int t = 0; t < d; ++t) S.A[i * nr + t] = R[i * nr + 1 + t];
        S.A[i * nr + d] = 1.0;
        S.b[i] = R[i * nr];
        S.flag[i] = 0;
    }
}

// the rows of S (dimension d, slots [0, m)) whose bit is set in s_kept into R, compacted in order; returns their number
__device__ inline int pj_compact(const TrLds &S, double *R, int m, int d, const unsigned long long *s_kept) {
    const int lane = threadIdx.x & 63, nr = d + 1;
    __syncthreads();
    int base = 0;
    for (int i0 = 0; i0 < m; i0 += 64) {
        const unsigned long long w = s_kept[i0 >> 6];
        const int i = i0 + lane;
        if (i < m && ((w >> lane) & 1ull)) {
            const int at = base + __popcll(w & ((1ull << lane) - 1ull));
            R[at * nr] = S.b[i];
            for (int t = 0; t < d; ++t) R[at * nr + 1 + t] = S.A[i * nr + t];
        }
        base += __popcll(w);
    }
    __syncthreads();
    return base;
}

__global__ void __launch_bounds__(64) k_project_rows(ProjectArgs a) {
    extern __shared__ double pj_smem[];
    __shared__ unsigned long long s_kept[RD_WORDS];
    __shared__ unsigned short s_pi[PJ_MAX_ROWS], s_ni[PJ_MAX_ROWS];
    const int lane = threadIdx.x & 63, n = a.n, m_lds = a.m_lds;
    const long long q = blockIdx.x;
    if (q >= a.n_poly) return;
    double *R = pj_smem + pj_s_bytes(m_lds, n) / 8;
    const long long r0 = a.row_off[q];
    const double tol = a.tol;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long pivots = 0, wide = 0, lps = 1, steps = 0, made = 0;
    int m = (int)(a.row_off[q + 1] - r0), d = n, status = PJ_OK, peak = 0;

    for (int i = lane; i < m * (n + 1); i += 64) R[i] = a.ef[r0 * (n + 1) + i];
    TrLds S = tr_lds(pj_smem, m_lds, d);
    if (lane < TR_D) S.x[lane] = (lane < n && a.start) ? a.start[q * n + lane] : 0.0;
    __syncthreads();
    pj_fill(S, R, m, d);
    int st = ov_radius(S, m, d, tol, pivots);
    wide += st == TR_UNBOUNDED || st == TR_CAPPED;
    if (st == TR_OPTIMAL && !(S.x[d] > tol)) status = PJ_THIN;
    double px = lane < d ? S.x[lane] : 0.0;
    if (status == PJ_OK && a.n_elim == 0) {
        if (lane < RD_WORDS) s_kept[lane] = 0ull;
        rd_row_loop<true>(S, m, d, tol, px, pivots, lps, wide, s_kept);
        m = pj_compact(S, R, m, d, s_kept);
    }

    for (int step = 0; step < a.n_elim && status == PJ_OK; ++step) {
        const int j = d - 1, nro = d + 1, nrn = d;   // row strides: the old rows in R and S.A of the new dimension d - 1 alike
        __syncthreads();
        S = tr_lds(pj_smem, m_lds, d - 1);
        // classes; the rows of Z
        int nz = 0, np = 0, nn = 0;
        for (int i0 = 0; i0 < m; i0 += 64) {
            const int i = i0 + lane;
            const double c = i < m ? R[i * nro + 1 + j] : 0.0;
            const bool is_p = i < m && c > PJ_ZERO_COEF, is_n = i < m && c < -PJ_ZERO_COEF, is_z = i < m && !is_p && !is_n;
            const unsigned long long bz = __ballot(is_z), bp = __ballot(is_p), bn = __ballot(is_n);
            if (is_p) s_pi[np + __popcll(bp & below)] = (unsigned short)i;
            if (is_n) s_ni[nn + __popcll(bn & below)] = (unsigned short)i;
            if (is_z) {
                const int at = nz + __popcll(bz & below);
                double scale = 1.0;
                if (c != 0.0) {
                    double ss = 0.0;
                    for (int t = 0; t < j; ++t) ss = fma(R[i * nro + 1 + t], R[i * nro + 1 + t], ss);
                    scale = sqrt(ss);
                }
                for (int t = 0; t < j; ++t) S.A[at * nrn + t] = R[i * nro + 1 + t] / scale;
                S.A[at * nrn + j] = 1.0;
                S.b[at] = R[i * nro] / scale;
                S.flag[at] = 0;
            }
            nz += __popcll(bz); np += __popcll(bp); nn += __popcll(bn);
        }
        const int n_pairs = (np && nn) ? np * nn : 0, total = nz + n_pairs;
        ++steps;
        peak = max(peak, total);
        if (total > min(PJ_MAX_ROWS, m_lds)) { status = PJ_TOO_LARGE; break; }   // m_lds: never below what a step can make (the host's bound)
        made += total;
        __syncthreads();
        // combinations
        int n_zero = 0;
        bool empty = false;
        for (int i = lane; i < n_pairs; i += 64) {
            const int p = s_pi[i / nn], r = s_ni[i % nn], at = nz + i;
            const double cp = R[p * nro + 1 + j], cq = -R[r * nro + 1 + j];   // both > 0
            double ss = 0.0;
            for (int t = 0; t < j; ++t) {
                const double v = cq * R[p * nro + 1 + t] + cp * R[r * nro + 1 + t];
                S.A[at * nrn + t] = v;
                ss = fma(v, v, ss);
            }
            const double rhs = cq * R[p * nro] + cp * R[r * nro], nrm = sqrt(ss);
            if (nrm <= PJ_ZERO_NORM) {
                ++n_zero;
                empty = empty || rhs < -tol;
                for (int t = 0; t <= j; ++t) S.A[at * nrn + t] = 0.0;
                S.b[at] = INFINITY;
                S.flag[at] = 2;
            } else {
                for (int t = 0; t < j; ++t) S.A[at * nrn + t] /= nrm;
                S.A[at * nrn + j] = 1.0;
                S.b[at] = rhs / nrm;
                S.flag[at] = 0;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) n_zero += __shfl_xor(n_zero, off);
        d = j;
        m = total;
        if (__any(empty)) { status = PJ_THIN; break; }
        if (total - n_zero == 0) { status = PJ_WHOLE; break; }
        // reduce
        if (lane >= d) px = 0.0;
        if (lane < TR_D) S.x[lane] = px;
        if (lane < RD_WORDS) s_kept[lane] = 0ull;
        st = ov_radius(S, m, d, tol, pivots);
        ++lps;
        wide += st == TR_UNBOUNDED || st == TR_CAPPED;
        if (st == TR_OPTIMAL && !(S.x[d] > tol)) { status = PJ_THIN; break; }
        px = lane < d ? S.x[lane] : 0.0;
        rd_row_loop<true>(S, m, d, tol, px, pivots, lps, wide, s_kept);
        m = pj_compact(S, R, m, d, s_kept);
    }

    if (status == PJ_OK && m > a.out_cap) status = PJ_TOO_LARGE;
    if (status == PJ_OK) {
        double *out = a.out_rows + q * (long long)a.out_cap * (d + 1);
        for (int i = lane; i < m * (d + 1); i += 64) out[i] = R[i];
        if (a.point && lane < d) a.point[q * d + lane] = px;
    }
    if (lane == 0) {
        a.status[q] = status;
        a.n_out[q] = status == PJ_OK ? m : 0;
        a.wide[q] = (int32_t)wide;
        a.peak[q] = peak;
        atomicAdd(a.counters + 0, 1ull);
        atomicAdd(a.counters + 1, status == PJ_THIN ? 1ull : 0ull);
        atomicAdd(a.counters + 2, status == PJ_WHOLE ? 1ull : 0ull);
        atomicAdd(a.counters + 3, status == PJ_TOO_LARGE ? 1ull : 0ull);
        atomicAdd(a.counters + 4, steps);
        atomicAdd(a.counters + 5, made);
        atomicAdd(a.counters + 6, lps);
        atomicAdd(a.counters + 7, pivots);
        atomicAdd(a.counters + 8, wide);
    }
}

}  // namespace mpc
