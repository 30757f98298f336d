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
// The simplex (tr_simplex): the working set holds n_t "rows", real rows of P^_j or pseudo rows (fixed coordinates, free to move either
// way), with the columns of the inverse basis d_k in LDS (B d_k = e_k).  Slot k's rate mu_k = c.d_k; a pseudo slot enters when
// |mu_k| / |d_k| > 1e-11, a real slot when mu_k / |d_k| > 1e-11 (the largest normalised rate first, pseudo slots before real ones).
// Ratio test over the rows outside the set (lanes over rows, slacks clamped at 0), ties to the lowest row; no blocking row: unbounded.
// A run that reaches TR_PIVOT_CAP pivots reports "unbounded" as well: a wider bound than the true one never costs exactness.
#pragma once
#include <stdint.h>

namespace mpc {

constexpr int TR_MAX_NT = 16, TR_MAX_ROWS = 256, TR_D = TR_MAX_NT + 1, TR_PIVOT_CAP = 400, TR_STACK = 8;
constexpr double TR_RATE_EPS = 1e-11, TR_RATE_G = 1e-12, TR_PHASE1_EPS = 1e-9, TR_ALLOW = 1e-9;

// LDS of one wavefront (workgroup of 64): rows A[m][n_t + 1] (column n_t = -1 for phase 1), b[m], flags, inverse basis, state
struct TrLds {
    double *A, *b, *D, *x, *p, *c, *box;   // D: [TR_D][TR_D], slot k at D[k * TR_D + i]; box: [2][TR_D] lower, upper
    int *flag, *W;                         // flag[r]: 0 free row, 1 in the working set, 2 dropped (zero row)
};

__host__ __device__ inline size_t tr_lds_bytes(int m_max, int nt) {
    return (size_t)m_max * (nt + 2) * 8 + (size_t)(TR_D * TR_D + 5 * TR_D) * 8 + (size_t)(m_max + TR_D) * 4;
}

__device__ inline TrLds tr_lds(double *base, int m_max, int nt) {
    TrLds S;
    S.A = base;
    S.b = S.A + (size_t)m_max * (nt + 1);
    S.D = S.b + m_max;
    S.x = S.D + TR_D * TR_D;
    S.p = S.x + TR_D;
    S.c = S.p + TR_D;
    S.box = S.c + TR_D;
    S.flag = reinterpret_cast<int *>(S.box + 2 * TR_D);
    S.W = S.flag + m_max;
    return S;
}

// the unit rows of P^_j: a = E_i / |E_i|, b = (f_i + tol max(1, |E_i|)) / |E_i|; a zero row is dropped (or empties the set).
// Returns 1 when a zero row empties the polytope.
__device__ inline int tr_load(const TrLds &S, const double *ef, long long r0, int m, int nt, double tol) {
    const int lane = threadIdx.x & 63;
    int empty = 0;
    for (int i = lane; i < m; i += 64) {
        const double *row = ef + (r0 + i) * (long long)(nt + 1);
        double nn = 0.0;
        for (int t = 0; t < nt; ++t) nn = fma(row[1 + t], row[1 + t], nn);
        const double nrm = sqrt(nn), rhs = row[0] + tol * fmax(1.0, nrm);
        if (nrm == 0.0) {
            S.flag[i] = 2;
            if (rhs < 0.0) empty = 1;
            for (int t = 0; t <= nt; ++t) S.A[i * (nt + 1) + t] = 0.0;
            S.b[i] = 0.0;
        } else {
            S.flag[i] = 0;
            for (int t = 0; t < nt; ++t) S.A[i * (nt + 1) + t] = row[1 + t] / nrm;
            S.A[i * (nt + 1) + nt] = -1.0;
            S.b[i] = rhs / nrm;
        }
    }
    __syncthreads();
    return __any(empty) ? 1 : 0;
}

// working set of pseudo rows at the current point: D = I (dimension d), W = -1, no row in the set
__device__ inline void tr_reset_basis(const TrLds &S, int m, int d) {
    const int lane = threadIdx.x & 63;
    if (lane < TR_D) {
        S.W[lane] = -1;
        for (int i = 0; i < TR_D; ++i) S.D[lane * TR_D + i] = (i == lane && lane < d) ? 1.0 : 0.0;
    }
    for (int i = lane; i < m; i += 64) if (S.flag[i] == 1) S.flag[i] = 0;
    __syncthreads();
}

enum { TR_OPTIMAL = 0, TR_UNBOUNDED = 1, TR_CAPPED = 2, TR_REACHED = 3 };

// minimise S.c . x over the rows from the current point and working set.  d = n_t (phase 2) or n_t + 1 (phase 1: c = e_{n_t},
// the run ends as soon as x_{n_t} reaches 0).  x moves only to feasible points; on UNBOUNDED / CAPPED x is the last point reached.
__device__ inline int tr_simplex(const TrLds &S, int m, int nt, int d, bool phase1, unsigned long long &pivots) {
    const int lane = threadIdx.x & 63, stride = nt + 1;
    for (int it = 0; it < TR_PIVOT_CAP; ++it) {
        // 1. entering slot
        double key = -1.0, sgn = 1.0;
        int slot = -1;
        if (lane < d) {
            double mu = 0.0, dd = 0.0;
            for (int i = 0; i < d; ++i) { const double v = S.D[lane * TR_D + i]; mu = fma(S.c[i], v, mu); dd = fma(v, v, dd); }
            const double rate = dd > 0.0 ? mu / sqrt(dd) : 0.0;
            if (S.W[lane] < 0) { if (fabs(rate) > TR_RATE_EPS) { key = 4.0 + fabs(rate); slot = lane; sgn = rate > 0.0 ? 1.0 : -1.0; } }
            else if (rate > TR_RATE_EPS) { key = rate; slot = lane; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ok = __shfl_xor(key, off);
            const int os = __shfl_xor(slot, off);
            if (os >= 0 && (slot < 0 || ok > key || (ok == key && os < slot))) { key = ok; slot = os; }
        }
        if (slot < 0) return TR_OPTIMAL;
        sgn = __shfl(sgn, slot);
        // 2. direction p = -sgn d_slot
        if (lane < d) S.p[lane] = -sgn * S.D[slot * TR_D + lane];
        __syncthreads();
        // 3. ratio test (ties to the lowest row; -2: phase 1 reaches x_{n_t} = 0, preferred on a tie)
        double tbest = INFINITY;
        int rbest = -1;
        for (int r = lane; r < m; r += 64) {
            if (S.flag[r]) continue;
            double g = 0.0, ax = 0.0;
            for (int i = 0; i < d; ++i) { const double a = S.A[r * stride + i]; g = fma(a, S.p[i], g); ax = fma(a, S.x[i], ax); }
            if (g > TR_RATE_G) {
                const double t = fmax(S.b[r] - ax, 0.0) / g;
                if (t < tbest || (t == tbest && r < rbest)) { tbest = t; rbest = r; }
            }
        }
        if (phase1 && lane == 0 && S.p[nt] < 0.0) {
            const double t = S.x[nt] / -S.p[nt];
            if (t <= tbest) { tbest = t; rbest = -2; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ot = __shfl_xor(tbest, off);
            const int orow = __shfl_xor(rbest, off);
            if (orow != -1 && (rbest == -1 || ot < tbest || (ot == tbest && orow < rbest))) { tbest = ot; rbest = orow; }
        }
        if (rbest == -1) return TR_UNBOUNDED;
        // 4. move
        __syncthreads();
        if (lane < d) S.x[lane] = fma(tbest, S.p[lane], S.x[lane]);
        if (rbest == -2) {
            if (lane == 0) S.x[nt] = 0.0;
            __syncthreads();
            return TR_REACHED;
        }
        // 5. row rbest replaces the slot: d_k' = d_k / alpha_k, d_j' = d_j - alpha_j d_k'
        double dk[TR_D];
        double alpha = 0.0;
#pragma unroll
        for (int i = 0; i < TR_D; ++i) dk[i] = i < d ? S.D[slot * TR_D + i] : 0.0;
        if (lane < d)
            for (int i = 0; i < d; ++i) alpha = fma(S.A[rbest * stride + i], S.D[lane * TR_D + i], alpha);
        const double ak = __shfl(alpha, slot);
        __syncthreads();
        if (lane < d) {
#pragma unroll
            for (int i = 0; i < TR_D; ++i) {
                if (i >= d) continue;
                const double nk = dk[i] / ak;
                S.D[lane * TR_D + i] = lane == slot ? nk : fma(-alpha, nk, S.D[lane * TR_D + i]);
            }
        }
        if (lane == 0) {
            const int old = S.W[slot];
            if (old >= 0) S.flag[old] = 0;
            S.flag[rbest] = 1;
            S.W[slot] = rbest;
        }
        __syncthreads();
        ++pivots;
    }
    return TR_CAPPED;
}

// a feasible point of the rows (phase 1 from theta = 0 in (theta, t) with rows a.theta - t <= b), left in x[0..nt) with a fresh
// phase-2 working set; returns false when the polytope is empty (min t > TR_PHASE1_EPS, or the run was capped)
__device__ inline bool tr_feasible(const TrLds &S, int m, int nt, unsigned long long &pivots) {
    const int lane = threadIdx.x & 63;
    double worst = 0.0;
    for (int r = lane; r < m; r += 64) if (!S.flag[r]) worst = fmax(worst, -S.b[r]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) worst = fmax(worst, __shfl_xor(worst, off));
    if (lane < TR_D) { S.x[lane] = lane == nt ? worst : 0.0; S.c[lane] = lane == nt ? 1.0 : 0.0; }
    __syncthreads();
    bool ok = true;
    if (worst > 0.0) {
        tr_reset_basis(S, m, nt + 1);
        const int st = tr_simplex(S, m, nt, nt + 1, true, pivots);
        ok = st == TR_REACHED || (st == TR_OPTIMAL && S.x[nt] <= TR_PHASE1_EPS);
        __syncthreads();
        if (lane == 0) S.x[nt] = 0.0;
    }
    tr_reset_basis(S, m, nt);
    return ok;
}

__device__ inline double tr_dot_x(const TrLds &S, int nt) {
    double v = 0.0;
    for (int t = 0; t < nt; ++t) v = fma(S.c[t], S.x[t], v);
    return v;
}

// c = sign * plane normal (lanes t < nt), then min c.x; returns min or -inf
__device__ inline double tr_min_plane(const TrLds &S, const double *nrm, double sign, int m, int nt, unsigned long long &pivots,
                                      unsigned long long &capped) {
    const int lane = threadIdx.x & 63;
    __syncthreads();
    if (lane < TR_D) S.c[lane] = lane < nt ? sign * nrm[lane] : 0.0;
    __syncthreads();
    const int st = tr_simplex(S, m, nt, nt, false, pivots);
    if (st == TR_CAPPED) ++capped;
    return st == TR_OPTIMAL ? tr_dot_x(S, nt) : -INFINITY;
}

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
        // bounding box: 2 n_t LPs
        for (int t = 0; t < nt; ++t) {
            __syncthreads();
            if (lane < TR_D) S.c[lane] = lane == t ? 1.0 : 0.0;
            __syncthreads();
            int st = tr_simplex(S, m, nt, nt, false, pivots);
            capped += st == TR_CAPPED;
            const double lo = st == TR_OPTIMAL ? S.x[t] : -INFINITY;
            __syncthreads();
            if (lane < TR_D) S.c[lane] = lane == t ? -1.0 : 0.0;
            __syncthreads();
            st = tr_simplex(S, m, nt, nt, false, pivots);
            capped += st == TR_CAPPED;
            const double hi = st == TR_OPTIMAL ? S.x[t] : INFINITY;
            if (lane == 0) { S.box[t] = lo; S.box[TR_D + t] = hi; }
            lps += 2;
        }
        __syncthreads();
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
template <int NT>
__global__ void __launch_bounds__(256) k_locate_tree(long long m, int nt, int nx, const double *__restrict__ planes,
                                                     const int32_t *__restrict__ node_plane, const int32_t *__restrict__ node_child,
                                                     const double *__restrict__ node_tau, const long long *__restrict__ node_off,
                                                     const int32_t *__restrict__ items, const long long *__restrict__ row_off,
                                                     const double *__restrict__ ef, const double *__restrict__ xlaw,
                                                     const double *__restrict__ Q, const double *__restrict__ cvec, const double *__restrict__ H,
                                                     const double *__restrict__ theta, double tol, int overlapping, int inclusive,
                                                     long long *__restrict__ region_out) {
    __shared__ int stack[TR_STACK][256];
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const int nr = nt + 1;
    double th[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) th[t] = t < nt ? theta[p * nt + t] : 0.0;
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
                stack[sp++][threadIdx.x] = node_child[2 * node + 1];
            }
            node = go_plus ? node_child[2 * node] : node_child[2 * node + 1];
        }
        if (overflow) break;
        for (long long i = node_off[node]; i < node_off[node + 1]; ++i) {
            const long long r = items[i];
            if (!overlapping && found >= 0 && r >= found) break;   // ascending lists: nothing earlier is left in this leaf
            bool inside = true;
            for (long long k = row_off[r]; k < row_off[r + 1] && inside; ++k) inside = loc_row_inside<NT>(ef + k * nr, th, nt, tol, inclusive);
            if (!inside) continue;
            if (!overlapping) { found = r; break; }
            const double obj = loc_objective<NT>(xlaw + (size_t)r * nx * nr, nx, nt, th, cvec, H, Q);
            if (obj < best || (obj == best && r > found)) { best = obj; found = r; }
        }
        if (sp == 0) break;
        node = stack[--sp][threadIdx.x];
    }
    region_out[p] = overflow ? -2 : found;
}

}  // namespace mpc
