// support.hpp -- support functions of polytopes (gfx950): h_P(d) = max {d.x : x in P} for lists of directions; DESIGN §3.28.
//
// A polytope arrives as unit rows [o | n] (|n| = 1, {theta : n.theta <= o}), at most SF_MAX_ROWS of them; its directions are rows
// dir_off[q] .. dir_off[q + 1] of dirs [n_dir][n_t].  Every LP is a run of the wavefront vertex simplex of simplex.hpp over rows in LDS;
// one WAVEFRONT (workgroup of 64) per item.  An item is (polytope q, first direction, count): at most SF_BLOCK consecutive directions
// of q, listed by the host, so a polytope with many directions spreads over the CUs.  A polytope without directions has one item.
//
//   k_support_rows  LDS rows [0, m): the polytope P.
//     interior point  the thin test of k_reduce_rows (reduce.hpp): radius(P) from start[q] (the origin without one), the run stops once
//                     t > tol.  Optimal with t <= tol: P is THIN, every direction of the item gets value = arg = NaN and no LP runs.
//                     Otherwise the theta where the run ended is p_q, kept in registers (lane i holds theta_i).  An unbounded or
//                     capped radius run is not thin and sets wide[q] = 1.  A run ends unbounded only while t <= tol, where theta need
//                     not lie in P: p_q is then moved along the ray the run found, which no row blocks, to t = tol + 1, a point of P
//                     of that radius.  A capped run with t >= 0 goes on from the point reached; with t < 0 no point of P is known
//                     and every direction of q gets value +inf, arg NaN and CAPPED without an LP.  Every item of q
//                     repeats this run and gets the same bits; the item that holds q's first direction (or q's only item) writes
//                     poly_status, wide and point, and counts the polytope and its radius LP.
//     one direction   d == 0 in every entry: value 0, arg p_q, no LP.  Otherwise c = d / |d| (d scaled by a power of two, then |d|^2 by fma over ascending t), x = p_q,
//                     tr_reset_basis, tr_min_plane with sign -1 on c.  Optimal: arg = x, value = sum over ascending t of
//                     fma(d_t, x_t, .), the objective of a feasible point in the units of d.  Unbounded: value +inf, arg the last point
//                     reached.  Pivot cap: value +inf (a bound, not a value), arg the last point reached.
//     independence    every run starts from p_q with a fresh basis, so a direction's result depends on (rows, start, tol, d) alone:
//                     not on its place in the list, not on the item it falls in, not on SF_BLOCK.
//   The only atomics are the counters; no floating-point atomics: a rerun gives the same bits.
#pragma once
#include <stdint.h>

#include "overlap.hpp"

namespace mpc {

constexpr int SF_MAX_ROWS = 512, SF_BLOCK = 64;
enum { SF_OK = 0, SF_UNBOUNDED = 1, SF_CAPPED = 2, SF_THIN = 3 };

struct SupportArgs {
    int nt, m_max;                        // m_max: LDS rows, at least the rows of every polytope
    long long n_items;
    const long long *row_off;
    const double *ef;                     // unit [o | n]
    const long long *dir_off;             // [n_poly + 1]
    const double *dirs;                   // [n_dir][nt]
    const int32_t *item_poly, *item_count;
    const long long *item_first;          // the item's first direction, a row of dirs
    const double *start;                  // [n_poly][nt] where the radius run starts, or nullptr: the origin
    double tol;
    double *value, *arg;                  // [n_dir], [n_dir][nt] or nullptr
    int32_t *dir_status, *poly_status, *wide;
    double *point;                        // [n_poly][nt], or nullptr
    unsigned long long *counters;         // polytopes, thin ones, directions, zero directions, LPs, pivots, unbounded or capped runs
};

__host__ __device__ inline size_t sf_lds_bytes(int m_max, int nt) { return 2 * TR_D * 8 + tr_lds_bytes(m_max, nt); }

__global__ void __launch_bounds__(64) k_support_rows(SupportArgs a) {
    extern __shared__ double sf_smem[];        // s_d, s_c, then the LDS of the simplex: sf_lds_bytes
    double *s_d = sf_smem, *s_c = sf_smem + TR_D;   // the direction as given, and scaled to unit length
    const int lane = threadIdx.x & 63, nt = a.nt;
    const long long it = blockIdx.x;
    if (it >= a.n_items) return;
    const TrLds S = tr_lds(sf_smem + 2 * TR_D, a.m_max, nt);
    const long long q = a.item_poly[it], first = a.item_first[it], r0 = a.row_off[q];
    const int count = a.item_count[it], m = (int)(a.row_off[q + 1] - r0);
    const bool owner = first == a.dir_off[q];
    unsigned long long pivots = 0, radius_pivots = 0, capped = 0, wide = 0, lps = 0, zero = 0;
    ov_load(S, a.ef, r0, m, nt, 0);
    if (lane < TR_D) S.x[lane] = (lane < nt && a.start) ? a.start[q * nt + lane] : 0.0;
    const int st = ov_radius(S, m, nt, a.tol, radius_pivots);
    const bool radius_wide = st == TR_UNBOUNDED || st == TR_CAPPED;
    const bool thin = st == TR_OPTIMAL && !(S.x[nt] > a.tol);
    const double t_end = S.x[nt];
    double px = lane < nt ? S.x[lane] : 0.0;
    // A run ends UNBOUNDED only while t <= tol, where theta need not lie in P yet (t < 0: it does not).  The ray it found (S.p, with
    // p_t > 0: it improves the objective) is blocked by no row: along it to t = tol + 1, a point of P of that radius.
    if (st == TR_UNBOUNDED && lane < nt) px = fma((a.tol + 1.0 - t_end) / S.p[nt], S.p[lane], px);
    const bool lost = st == TR_CAPPED && t_end < 0.0;     // the pivot cap before any point of P: no direction can run
    for (int j = 0; j < count; ++j) {
        const long long g = first + j;
        double val = NAN, xo = NAN;
        int ds = SF_THIN;
        if (lost) {
            val = INFINITY;
            ds = SF_CAPPED;
        } else if (!thin) {
            const double dv = lane < nt ? a.dirs[g * nt + lane] : 0.0;
            val = 0.0; xo = px; ds = SF_OK;
            if (!__any(dv != 0.0)) {
                ++zero;
            } else {
                __syncthreads();                       // the run before this one has read s_d and S.x
                if (lane < TR_D) { s_d[lane] = dv; S.x[lane] = px; }
                __syncthreads();
                // c = d / |d| with d scaled by a power of two first (exact: the same bits wherever |d|^2 is representable, and no
                // overflow or underflow anywhere else)
                double mx = fabs(dv);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
                const double e = scalbn(dv, -ilogb(mx));
                double nn = 0.0;
                for (int t = 0; t < nt; ++t) { const double et = __shfl(e, t); nn = fma(et, et, nn); }
                if (lane < TR_D) s_c[lane] = e / sqrt(nn);
                tr_reset_basis(S, m, nt);
                const unsigned long long before = capped;
                const double lo = tr_min_plane(S, s_c, -1.0, m, nt, pivots, capped);   // min -c.x; -inf when unbounded or capped
                ++lps;
                if (isinf(lo)) {
                    ds = capped != before ? SF_CAPPED : SF_UNBOUNDED;
                    val = INFINITY;
                    ++wide;
                } else {
                    for (int t = 0; t < nt; ++t) val = fma(s_d[t], S.x[t], val);
                }
                xo = lane < nt ? S.x[lane] : 0.0;
            }
        }
        if (a.arg && lane < nt) a.arg[g * nt + lane] = xo;
        if (lane == 0) { a.value[g] = val; a.dir_status[g] = ds; }
    }
    if (owner) {
        if (a.point && lane < nt) a.point[q * nt + lane] = px;
        if (lane == 0) { a.poly_status[q] = thin ? SF_THIN : SF_OK; a.wide[q] = radius_wide ? 1 : 0; }
    }
    if (lane == 0) {
        if (owner) {
            atomicAdd(a.counters + 0, 1ull);
            atomicAdd(a.counters + 1, thin ? 1ull : 0ull);
            lps += 1;
            pivots += radius_pivots;
            wide += radius_wide ? 1ull : 0ull;
        }
        atomicAdd(a.counters + 2, (unsigned long long)count);
        atomicAdd(a.counters + 3, zero);
        atomicAdd(a.counters + 4, lps);
        atomicAdd(a.counters + 5, pivots);
        atomicAdd(a.counters + 6, wide);
    }
}

}  // namespace mpc
