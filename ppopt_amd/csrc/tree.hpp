// tree.hpp -- binary search trees over a solution's hyperplanes for point location (gfx950); DESIGN §3.13.
//
// Every region j is classified against every plane s(theta) = n.theta - o (|n| = 1) through its EXPANDED polytope
//   P^_j = {theta : E_i theta <= f_i + tol max(1, |E_i|)},
// which holds the scan's membership set (raw rows, strict or inclusive, tol_q <= tol) and the exported code's (unit rows).  With
// lo_j = min s, hi_j = max s over P^_j and a band w: "+" iff lo_j >= -w, "-" iff hi_j <= w, straddling when neither or both hold.
//
//   k_tree_classify<0>  one WAVEFRONT per region: the region's unit rows in LDS, a feasible point by a phase-1 simplex, the bounding
//                       box of P^_j (2 n_t LPs), then for every plane the interval bound of s over the box (lane-parallel, 64 planes
//                       at a time) and, for the pairs the box cannot decide, min / max of s by the vertex simplex warm-started from the
//                       previous optimum.  Output: region-major bitsets plus[j][h / 64], minus[j][h / 64] (one ballot per 64 planes,
//                       no atomics), a feasible point per region (the warm start of mode 1) and counters.
//   k_tree_classify<1>  one wavefront per (node, region) pair of a level whose region lies on one side of the node's plane only: the
//                       exact LP bound (min s for "+", max s for "-"), widened by the rounding allowance, folded into tau by an
//                       atomic max of non-negative doubles (order-independent).
//   k_tree_split        one thread per (node, candidate plane): n+, n- over the node's region list, key (max(n+ + n0, n- + n0), n0, h).
//   k_tree_partition    one thread per (node, region): which children receive the region.
//   k_locate_tree       one lane per point: descent with a stack of 8 pending nodes in LDS, the leaf lists tested with the scan's
//                       own row test and objective (loc_row_inside / loc_objective, locate.hpp).  Overflow: -2, the host re-scans.
//
// The simplex and its LDS layout live in simplex.hpp.
#pragma once
#include <stdint.h>

#include "simplex.hpp"

namespace mpc {

constexpr int TR_STACK = 8;
constexpr double TR_ALLOW = 1e-9;

struct TreeClassifyArgs {
    int nt, m_max, n_planes, hw;
    long long n_regions;
    const long long *row_off;
    const double *ef;           // the locator's stacked [f | E]
    const double *planes;       // [n_planes][nt + 1]: unit [n | o]
    double tol, band;
    // mode 0
    unsigned long long *plus, *minus;   // [n_regions][hw]
    double *xs;                         // [n_regions][nt]: a feasible point of P^_j
    int32_t *empty;                     // [n_regions]
    // mode 1
    long long n_pairs;
    const int32_t *pair;                // [n_pairs][3]: node, region, side (0: "+" only -> tau-, 1: "-" only -> tau+)
    const int32_t *node_plane;          // [nodes of the level]
    unsigned long long *tau;            // [nodes of the level][2], non-negative doubles as bits
    unsigned long long *counters;       // pairs, box-decided pairs, LPs, pivots, capped runs
};

template <int MODE>
__global__ void __launch_bounds__(64) k_tree_classify(TreeClassifyArgs a) {
    extern __shared__ double tr_smem[];
    const int lane = threadIdx.x & 63, nt = a.nt;
    const long long item = blockIdx.x;
    const TrLds S = tr_lds(tr_smem, a.m_max, nt);
    unsigned long long pivots = 0, lps = 0, boxed = 0, capped = 0;
    if constexpr (MODE == 0) {
        const long long j = item;
        if (j >= a.n_regions) return;
        const long long r0 = a.row_off[j];
        const int m = (int)(a.row_off[j + 1] - r0);
        const int zero_empty = tr_load(S, a.ef, r0, m, nt, a.tol);
        const bool feasible = !zero_empty && tr_feasible(S, m, nt, pivots);
        if (!feasible) {   // an empty expanded polytope: straddles every plane (no bit set), never one-sided
            if (lane == 0) {
                a.empty[j] = 1;
                for (int t = 0; t < nt; ++t) a.xs[j * nt + t] = 0.0;
                atomicAdd(a.counters + 0, (unsigned long long)a.n_planes);
                atomicAdd(a.counters + 3, pivots);
            }
            return;
        }
        tr_box(S, m, nt, pivots, capped, lps);   // bounding box: 2 n_t LPs
        const double w = a.band;
        for (int cw = 0; cw < a.hw; ++cw) {
            const int h = cw * 64 + lane;
            const bool live = h < a.n_planes;
            // interval bound of s over the box: plus / minus in {0 no, 1 yes, 2 undecided}
            int plus = 0, minus = 0;
            if (live) {
                const double *pl = a.planes + (long long)h * (nt + 1);
                double lo = -pl[nt], hi = -pl[nt];
                for (int t = 0; t < nt; ++t) {
                    const double nv = pl[t];
                    if (nv > 0.0) { lo = fma(nv, S.box[t], lo); hi = fma(nv, S.box[TR_D + t], hi); }
                    else if (nv < 0.0) { lo = fma(nv, S.box[TR_D + t], lo); hi = fma(nv, S.box[t], hi); }
                }
                plus = lo >= -w ? 1 : (hi < -w ? 0 : 2);
                minus = hi <= w ? 1 : (lo > w ? 0 : 2);
                boxed += (plus != 2 && minus != 2);
            }
            unsigned long long open = __ballot(live && (plus == 2 || minus == 2));
            while (open) {
                const int l = __builtin_ctzll(open);
                open &= open - 1;
                const double *pl = a.planes + (long long)(cw * 64 + l) * (nt + 1);
                const double o = pl[nt];
                const int pl_l = __shfl(plus, l), mi_l = __shfl(minus, l);
                int np = pl_l, nm = mi_l;
                if (np == 2) {
                    const double lo = tr_min_plane(S, pl, 1.0, m, nt, pivots, capped) - o;
                    ++lps;
                    np = lo >= -w ? 1 : 0;
                    if (nm == 2 && lo > w) nm = 0;
                }
                if (nm == 2) {
                    const double hi = -tr_min_plane(S, pl, -1.0, m, nt, pivots, capped) - o;
                    ++lps;
                    nm = hi <= w ? 1 : 0;
                }
                if (lane == l) { plus = np; minus = nm; }
            }
            const unsigned long long pw = __ballot(live && plus == 1), mw = __ballot(live && minus == 1);
            if (lane == 0) { a.plus[j * a.hw + cw] = pw; a.minus[j * a.hw + cw] = mw; }
        }
        __syncthreads();
        if (lane < nt) a.xs[j * nt + lane] = S.x[lane];
        if (lane == 0) a.empty[j] = 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) boxed += __shfl_xor(boxed, off);
        if (lane == 0) {
            atomicAdd(a.counters + 0, (unsigned long long)a.n_planes);
            atomicAdd(a.counters + 1, boxed);
            atomicAdd(a.counters + 2, lps);
            atomicAdd(a.counters + 3, pivots);
            atomicAdd(a.counters + 4, capped);
        }
    } else {
        if (item >= a.n_pairs) return;
        const int node = a.pair[3 * item], side = a.pair[3 * item + 2];
        const long long j = a.pair[3 * item + 1];
        const long long r0 = a.row_off[j];
        const int m = (int)(a.row_off[j + 1] - r0);
        (void)tr_load(S, a.ef, r0, m, nt, a.tol);
        if (lane < TR_D) S.x[lane] = lane < nt ? a.xs[j * nt + lane] : 0.0;
        tr_reset_basis(S, m, nt);
        const double *pl = a.planes + (long long)a.node_plane[node] * (nt + 1);
        const double o = pl[nt];
        // side 0: min s; side 1: max s
        const double v = tr_min_plane(S, pl, side == 0 ? 1.0 : -1.0, m, nt, pivots, capped);
        double xn = 0.0;
        for (int t = 0; t < nt; ++t) xn += fabs(S.x[t]);
        const double allow = TR_ALLOW * (1.0 + fabs(o) + xn);
        double tau;
        if (v == -INFINITY) tau = INFINITY;
        else if (side == 0) tau = fmax(0.0, -(v - o)) + allow;
        else tau = fmax(0.0, -v - o) + allow;
        if (lane == 0) {
            atomicMax(a.tau + 2 * node + side, (unsigned long long)__double_as_longlong(tau));
            atomicAdd(a.counters + 2, 1ull);
            atomicAdd(a.counters + 3, pivots);
            atomicAdd(a.counters + 4, capped);
        }
    }
}

// every (node, candidate plane): n+ ("+" only), n- ("-" only) over the node's list; best key (max(n+ + n0, n- + n0), n0, h) per
// (node = blockIdx.x, chunk of planes = blockIdx.y).  Candidates: the planes of the node's regions (owner bit), or all planes when owner is NULL.
constexpr int TS_BLOCK = 256, TS_NONE = 0x7fffffff;
__global__ void __launch_bounds__(TS_BLOCK) k_tree_split(int n_planes, int hw, int chunk_len, const long long *__restrict__ node_off,
                                                         const int32_t *__restrict__ items, const unsigned long long *__restrict__ plus,
                                                         const unsigned long long *__restrict__ minus, const unsigned long long *__restrict__ owner,
                                                         int4 *__restrict__ partial) {
    __shared__ int s_key[TS_BLOCK / 64][3];
    const int node = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long i0 = node_off[node], i1 = node_off[node + 1];
    const int size = (int)(i1 - i0);
    const int h0 = blockIdx.y * chunk_len, h1 = min(h0 + chunk_len, n_planes);
    int bmx = TS_NONE, bn0 = TS_NONE, bh = TS_NONE;
    for (int h = h0 + threadIdx.x; h < h1; h += TS_BLOCK) {
        const int wd = h >> 6;
        const unsigned long long bit = 1ull << (h & 63);
        int np = 0, nm = 0;
        bool cand = owner == nullptr;
        for (long long i = i0; i < i1; ++i) {
            const long long q = (long long)items[i] * hw + wd;
            const bool p = plus[q] & bit, mn = minus[q] & bit;
            np += p && !mn;
            nm += mn && !p;
            if (owner) cand = cand || (owner[q] & bit);
        }
        if (!cand) continue;
        const int n0 = size - np - nm, mx = max(np, nm) + n0;
        if (mx < bmx || (mx == bmx && (n0 < bn0 || (n0 == bn0 && h < bh)))) { bmx = mx; bn0 = n0; bh = h; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int omx = __shfl_xor(bmx, off), on0 = __shfl_xor(bn0, off), oh = __shfl_xor(bh, off);
        if (omx < bmx || (omx == bmx && (on0 < bn0 || (on0 == bn0 && oh < bh)))) { bmx = omx; bn0 = on0; bh = oh; }
    }
    if (lane == 0) { s_key[wv][0] = bmx; s_key[wv][1] = bn0; s_key[wv][2] = bh; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < TS_BLOCK / 64; ++k) {
            const int omx = s_key[k][0], on0 = s_key[k][1], oh = s_key[k][2];
            if (omx < bmx || (omx == bmx && (on0 < bn0 || (on0 == bn0 && oh < bh)))) { bmx = omx; bn0 = on0; bh = oh; }
        }
        partial[(long long)node * gridDim.y + blockIdx.y] = make_int4(bmx, bn0, bh == TS_NONE ? -1 : bh, size);
    }
}

// side of every (node, region) item for the node's chosen plane: 1 "+" only, 2 "-" only, 0 both children
__global__ void __launch_bounds__(256) k_tree_partition(long long n_items, int hw, const int32_t *__restrict__ items,
                                                        const int32_t *__restrict__ item_plane, const unsigned long long *__restrict__ plus,
                                                        const unsigned long long *__restrict__ minus, int8_t *__restrict__ side) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const int h = item_plane[i];
    const long long q = (long long)items[i] * hw + (h >> 6);
    const unsigned long long bit = 1ull << (h & 63);
    const bool p = plus[q] & bit, m = minus[q] & bit;
    side[i] = (int8_t)(p && !m ? 1 : (m && !p ? 2 : 0));
}

// owner bits: region j has plane h (the region's (plane, side) list of the export)
__global__ void __launch_bounds__(256) k_tree_owner(long long n_entries, int hw, const int32_t *__restrict__ entry_region,
                                                    const int32_t *__restrict__ entry_plane, unsigned long long *__restrict__ owner) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_entries) return;
    const int h = entry_plane[i];
    atomicOr(owner + (long long)entry_region[i] * hw + (h >> 6), 1ull << (h & 63));
}

// Descent: node_plane[k] < 0 marks a leaf with regions items[node_off[k] .. node_off[k + 1]) (ascending).  The "+" child is visited
// if s >= -tau-, the "-" child if s <= tau+; the second child of a band goes on a stack of TR_STACK nodes per lane (LDS); a lane
// whose stack overflows returns -2 and the host hands the point to the list scan.
// The descent of one lane (shared by k_locate_tree and k_simulate, closed_loop.hpp): the region, -1 for none, -2 on a stack overflow.
// stack: LDS of TR_STACK x 256 ints, the lane's column threadIdx.x (blocks of 256).
template <int NT>
__device__ __forceinline__ long long loc_tree(const double (&th)[NT], int nt, int nx, const double *__restrict__ planes,
                                              const int32_t *__restrict__ node_plane, const int32_t *__restrict__ node_child,
                                              const double *__restrict__ node_tau, const long long *__restrict__ node_off,
                                              const int32_t *__restrict__ items, const long long *__restrict__ row_off,
                                              const double *__restrict__ ef, const double *__restrict__ xlaw, const double *__restrict__ Q,
                                              const double *__restrict__ cvec, const double *__restrict__ H, double tol, int overlapping,
                                              int inclusive, int *stack) {
    const int nr = nt + 1;
    long long found = -1;
    double best = INFINITY;
    int sp = 0, node = 0;
    bool overflow = false;
    for (;;) {
        int h;
        while ((h = node_plane[node]) >= 0) {
            const double *pl = planes + (long long)h * nr;
            double s = -pl[nt];
#pragma unroll
            for (int t = 0; t < NT; ++t) if (t < nt) s = fma(pl[t], th[t], s);
            const bool go_plus = s >= -node_tau[2 * node], go_minus = s <= node_tau[2 * node + 1];
            if (go_plus && go_minus) {
                if (sp == TR_STACK) { overflow = true; break; }
                stack[sp++ * 256 + threadIdx.x] = node_child[2 * node + 1];
            }
            node = go_plus ? node_child[2 * node] : node_child[2 * node + 1];
        }
        if (overflow) break;
        for (long long i = node_off[node]; i < node_off[node + 1]; ++i) {
            const long long r = items[i];
            if (!overlapping && found >= 0 && r >= found) break;   // ascending lists: nothing earlier is left in this leaf
            if (row_off[r + 1] <= row_off[r]) continue;   // the scan walks rows: a region without rows is never met, here neither
            bool inside = true;
            for (long long k = row_off[r]; k < row_off[r + 1] && inside; ++k) inside = loc_row_inside<NT>(ef + k * nr, th, nt, tol, inclusive);
            if (!inside) continue;
            if (!overlapping) { found = r; break; }
            const double obj = loc_objective<NT>(xlaw + (size_t)r * nx * nr, nx, nt, th, cvec, H, Q);
            if (obj < best || (obj == best && r > found)) { best = obj; found = r; }
        }
        if (sp == 0) break;
        --sp;
        node = stack[sp * 256 + threadIdx.x];
    }
    return overflow ? -2 : found;
}

template <int NT>
__global__ void __launch_bounds__(256) k_locate_tree(long long m, int nt, int nx, const double *__restrict__ planes,
                                                     const int32_t *__restrict__ node_plane, const int32_t *__restrict__ node_child,
                                                     const double *__restrict__ node_tau, const long long *__restrict__ node_off,
                                                     const int32_t *__restrict__ items, const long long *__restrict__ row_off,
                                                     const double *__restrict__ ef, const double *__restrict__ xlaw,
                                                     const double *__restrict__ Q, const double *__restrict__ cvec, const double *__restrict__ H,
                                                     const double *__restrict__ theta, double tol, int overlapping, int inclusive,
                                                     long long *__restrict__ region_out) {
    __shared__ int stack[TR_STACK * 256];
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    double th[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) th[t] = t < nt ? theta[p * nt + t] : 0.0;
    region_out[p] = loc_tree<NT>(th, nt, nx, planes, node_plane, node_child, node_tau, node_off, items, row_off, ef, xlaw, Q, cvec, H, tol, overlapping,
                                 inclusive, stack);
}

}  // namespace mpc
