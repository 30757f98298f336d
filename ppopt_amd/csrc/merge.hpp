// merge.hpp -- pairwise convexity tests of same-law regions for Solution.merge_regions (gfx950); DESIGN §3.14.
//
// Regions arrive as unit rows [o | n] (|n| = 1, region {theta : n.theta <= o}), at most MG_MAX_ROWS each.
//
//   k_merge_regions  one WAVEFRONT per region: the rows in LDS, a feasible point by the phase-1 simplex and the bounding box (2 n_t
//                    LPs, tr_box).  Output: xs[j][n_t], box[j][2][n_t] (lower, upper; +-inf where unbounded), status[j] (1: empty).
//   k_merge_pairs    one wavefront per candidate pair (P, Q), from the feasible points and boxes of k_merge_regions:
//     envelope       row r of P is valid for Q iff max over Q of (n_r.theta - o_r) <= tol max(1, |o_r|), and the same for the rows of
//                    Q over P.  Q's rows sit in LDS; 64 rows of P at a time, lane-parallel: valid if the bound over Q's box holds,
//                    not valid if Q's feasible point already breaks it, else an LP (max n_r.theta over Q, warm-started from the
//                    previous optimum).  An unbounded or capped LP: not valid.
//     convexity      P u Q is convex iff for every non-envelope row i of P and j of Q (Bemporad, Fukuda, Torrisi 2001)
//                      max t  s.t.  n_e.theta <= o_e + tol max(1, |o_e|) (e in env),  n_i.theta - o_i >= t,  n_j.theta - o_j >= t
//                    has t* <= tol.  The LP runs in (theta, t) from P's feasible point (feasible for the widened envelope) with
//                    t = min of the two reversed rows, and stops as soon as t > tol.  Unbounded or capped: not convex.
//     output         env_a[pair][MG_WORDS], env_b[pair][MG_WORDS] (bit r: row r is valid for the partner), verdict[pair] (1 convex),
//                    t_max[pair] (largest t reached; -inf without any convexity LP) and counters.  The only atomics are counters.
#pragma once
#include <stdint.h>

#include "simplex.hpp"

namespace mpc {

constexpr int MG_MAX_ROWS = 256, MG_WORDS = MG_MAX_ROWS / 64;

// feasible point and bounding box of every region
__global__ void __launch_bounds__(64) k_merge_regions(int nt, int m_max, long long n_regions, const long long *__restrict__ row_off,
                                                      const double *__restrict__ ef, double *__restrict__ xs, double *__restrict__ box,
                                                      int32_t *__restrict__ status, unsigned long long *__restrict__ counters) {
    extern __shared__ double mg_smem[];
    const int lane = threadIdx.x & 63;
    const long long j = blockIdx.x;
    if (j >= n_regions) return;
    const TrLds S = tr_lds(mg_smem, m_max, nt);
    const long long r0 = row_off[j];
    const int m = (int)(row_off[j + 1] - r0);
    unsigned long long pivots = 0, capped = 0, lps = 1;
    const int zero_empty = tr_load(S, ef, r0, m, nt, 0.0);
    const bool feasible = !zero_empty && tr_feasible(S, m, nt, pivots);
    if (feasible) tr_box(S, m, nt, pivots, capped, lps);
    if (lane < nt) {
        xs[j * nt + lane] = feasible ? S.x[lane] : 0.0;
        box[(2 * j) * nt + lane] = feasible ? S.box[lane] : INFINITY;
        box[(2 * j + 1) * nt + lane] = feasible ? S.box[TR_D + lane] : -INFINITY;
    }
    if (lane == 0) {
        status[j] = feasible ? 0 : 1;
        atomicAdd(counters + 0, lps);
        atomicAdd(counters + 1, pivots);
        atomicAdd(counters + 2, capped);
    }
}

struct MergePairArgs {
    int nt, m_max;                      // m_max: LDS rows, at least m_P + m_Q + 2 of every pair
    long long n_pairs;
    const long long *row_off;
    const double *ef;                   // [rows][nt + 1] unit [o | n]
    const double *xs, *box;             // of k_merge_regions
    const int32_t *pair_a, *pair_b;
    double tol;
    unsigned long long *env_a, *env_b;  // [n_pairs][MG_WORDS]
    int32_t *verdict;
    double *t_max;
    unsigned long long *counters;       // pairs, pairs whose envelope needed no LP, rows tested, rows decided without LP, LPs, pivots, capped
};

__global__ void __launch_bounds__(64) k_merge_pairs(MergePairArgs a) {
    extern __shared__ double mg_smem[];
    __shared__ unsigned long long s_env[2][MG_WORDS];
    const int lane = threadIdx.x & 63, nt = a.nt, nr = nt + 1;
    const long long q = blockIdx.x;
    if (q >= a.n_pairs) return;
    const TrLds S = tr_lds(mg_smem, a.m_max, nt);
    // P = a, Q = b (selected by ternaries, not by arrays: a runtime-indexed array would live in scratch)
    const long long reg_a = a.pair_a[q], reg_b = a.pair_b[q], r0_a = a.row_off[reg_a], r0_b = a.row_off[reg_b];
    const int m_a = (int)(a.row_off[reg_a + 1] - r0_a), m_b = (int)(a.row_off[reg_b + 1] - r0_b);
    const double tol = a.tol;
    unsigned long long pivots = 0, capped = 0, lps = 0, tested = 0, screened = 0;
    // 1. envelope: side 0 tests P's rows over Q, side 1 Q's rows over P
    for (int side = 0; side < 2; ++side) {
        const int mX = side ? m_a : m_b, mY = side ? m_b : m_a;      // rows of Y (= side), maximised over X
        const long long gx = side ? reg_a : reg_b, rx = side ? r0_a : r0_b, ry = side ? r0_b : r0_a;
        __syncthreads();
        for (int i = lane; i < mX; i += 64) {
            const double *row = a.ef + (rx + i) * nr;
            for (int t = 0; t < nt; ++t) S.A[i * nr + t] = row[1 + t];
            S.A[i * nr + nt] = 0.0;
            S.b[i] = row[0];
            S.flag[i] = 0;
        }
        if (lane < TR_D) S.x[lane] = lane < nt ? a.xs[gx * nt + lane] : 0.0;
        tr_reset_basis(S, mX, nt);
        const double *lo = a.box + (2 * gx) * nt, *hi = a.box + (2 * gx + 1) * nt, *xp = a.xs + gx * nt;
        for (int cw = 0; cw < MG_WORDS; ++cw) {
            const int r = cw * 64 + lane;
            const bool live = r < mY;
            int state = 0;   // 1 valid, 0 not valid, 2 undecided
            if (live) {
                const double *row = a.ef + (ry + r) * nr;
                const double o = row[0], thr = tol * fmax(1.0, fabs(o));
                double bound = -o, at = -o;
                for (int t = 0; t < nt; ++t) {
                    const double n = row[1 + t];
                    if (n > 0.0) bound = fma(n, hi[t], bound);
                    else if (n < 0.0) bound = fma(n, lo[t], bound);
                    at = fma(n, xp[t], at);
                }
                state = bound <= thr ? 1 : (at > thr ? 0 : 2);
            }
            tested += live;
            screened += live && state != 2;
            unsigned long long open = __ballot(live && state == 2);
            while (open) {
                const int l = __builtin_ctzll(open);
                open &= open - 1;
                const double *row = a.ef + (ry + cw * 64 + l) * nr;
                const double o = row[0];
                const double mx = -tr_min_plane(S, row + 1, -1.0, mX, nt, pivots, capped);   // +inf when unbounded or capped
                ++lps;
                if (lane == l) state = mx - o <= tol * fmax(1.0, fabs(o)) ? 1 : 0;
            }
            const unsigned long long w = __ballot(live && state == 1);
            if (lane == 0) s_env[side][cw] = w;
        }
    }
    __syncthreads();
    // 2. the widened envelope in LDS: P's valid rows, then Q's; rows m_env, m_env + 1 are the reversed pair of each LP
    int m_env = 0;
    for (int side = 0; side < 2; ++side) {
        for (int cw = 0; cw < MG_WORDS; ++cw) {
            const int r = cw * 64 + lane;
            const bool in = r < (side ? m_b : m_a) && ((s_env[side][cw] >> lane) & 1ull);
            const unsigned long long bal = __ballot(in);
            if (in) {
                const int pos = m_env + __popcll(bal & ((1ull << lane) - 1ull));
                const double *row = a.ef + ((side ? r0_b : r0_a) + r) * nr;
                for (int t = 0; t < nt; ++t) S.A[pos * nr + t] = row[1 + t];
                S.A[pos * nr + nt] = 0.0;
                S.b[pos] = row[0] + tol * fmax(1.0, fabs(row[0]));
                S.flag[pos] = 0;
            }
            m_env += __popcll(bal);
        }
    }
    const int m = m_env + 2;
    if (lane < 2) S.flag[m_env + lane] = 0;
    __syncthreads();
    int verdict = 1;
    double tmax = -INFINITY;
    const double *xp = a.xs + reg_a * nt;
    for (int i = 0; i < m_a && verdict; ++i) {
        if ((s_env[0][i >> 6] >> (i & 63)) & 1ull) continue;
        const double *ri = a.ef + (r0_a + i) * nr;
        for (int j = 0; j < m_b; ++j) {
            if ((s_env[1][j >> 6] >> (j & 63)) & 1ull) continue;
            const double *rj = a.ef + (r0_b + j) * nr;
            __syncthreads();
            if (lane < nt) {
                S.A[m_env * nr + lane] = -ri[1 + lane];
                S.A[(m_env + 1) * nr + lane] = -rj[1 + lane];
            }
            if (lane == 0) {
                S.A[m_env * nr + nt] = 1.0;
                S.A[(m_env + 1) * nr + nt] = 1.0;
                S.b[m_env] = -ri[0];
                S.b[m_env + 1] = -rj[0];
            }
            if (lane < TR_D) {
                double v = 0.0;
                if (lane < nt) v = xp[lane];
                else if (lane == nt) {
                    double si = -ri[0], sj = -rj[0];
                    for (int t = 0; t < nt; ++t) { si = fma(ri[1 + t], xp[t], si); sj = fma(rj[1 + t], xp[t], sj); }
                    v = fmin(si, sj);
                }
                S.x[lane] = v;
                S.c[lane] = lane == nt ? -1.0 : 0.0;
            }
            tr_reset_basis(S, m, nt + 1);
            const int st = tr_simplex(S, m, nt, nt + 1, false, pivots, tol);
            ++lps;
            capped += st == TR_CAPPED;
            const double t = (st == TR_OPTIMAL || st == TR_REACHED) ? S.x[nt] : INFINITY;
            tmax = fmax(tmax, t);
            if (!(t <= tol)) { verdict = 0; break; }
        }
    }
    __syncthreads();
    if (lane < MG_WORDS) {
        a.env_a[q * MG_WORDS + lane] = s_env[0][lane];
        a.env_b[q * MG_WORDS + lane] = s_env[1][lane];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { tested += __shfl_xor(tested, off); screened += __shfl_xor(screened, off); }
    if (lane == 0) {
        a.verdict[q] = verdict;
        a.t_max[q] = tmax;
        atomicAdd(a.counters + 0, 1ull);
        atomicAdd(a.counters + 1, tested == screened ? 1ull : 0ull);
        atomicAdd(a.counters + 2, tested);
        atomicAdd(a.counters + 3, screened);
        atomicAdd(a.counters + 4, lps);
        atomicAdd(a.counters + 5, pivots);
        atomicAdd(a.counters + 6, capped);
    }
}

}  // namespace mpc
