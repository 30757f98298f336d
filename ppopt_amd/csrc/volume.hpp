// volume.hpp -- volumes and centroids of a batch of polytopes from their vertex lists and incidence masks (gfx950); DESIGN §3.17.
//
// The boundary triangulation of Cohen & Hickey on the face lattice, which the incidence gives without arithmetic.  A face is a set S of
// vertices (a bitset of W = ceil(V / 64) words) with its dimension d; its apex is its lowest vertex.  The facets of S are the maximal
// proper non-empty sets among {S & C_r}, C_r the vertices tight on row r; equal sets count once (the lowest r).  vol_d(S) is the sum of
// vol_{d-1}(F) over the facets F of S without apex(S), the apex joining a chain; a face of dimension 0 closes a simplex of the chain and
// its vertex.
//   k_volume_rowsets  one workgroup per polytope: C_r from the vertex incidence, stored by word, Ct[w][r] (lanes over rows read
//                     neighbouring addresses).
//   k_volume_walk     one WAVEFRONT per (polytope, row r).  The wave first tests whether C_r is a facet of the polytope without vertex 0;
//                     if so it walks the faces below it depth first.  The stack (one bitset, the candidate rows and a "facet found" flag
//                     per level) is in LDS, and so are the Ct of the polytope when they fit (c_in_lds).  Lanes run over rows for the
//                     candidate masks and the maximality test, over words for the set operations.
//                     The determinant is kept in eliminated form along the chain: apex k contributes the row a_k - a_0, eliminated
//                     against the rows before it with the pivot in the column of its largest remaining entry (partial pivoting of the
//                     transposed matrix, fp64); a leaf eliminates one more row, |det| = the product of the pivots.  A face shares the
//                     rows of its chain with every simplex below it.  Lane c holds coordinate c.
//                     The wave writes its sums (volume n!, first moment n! (n + 1), simplices, status) to the slot of its row.
//   k_volume_reduce   one thread per polytope adds the slots of its rows in row order: no floating-point atomics, the same bits twice.
// Guards: a face of dimension > 1 without a facet that avoids its apex, an edge that does not hold two vertices, a vertex face that does
// not hold one, or a polytope without any simplex -> VOL_INCONSISTENT (the incidence was blurred by a vertex merge).  More than
// max_simplices simplices in one polytope -> VOL_TOO_LARGE: every wave counts its own, and adds them to the polytope's counter (an
// integer atomic) every VOL_BATCH simplices to stop early.
//
// Second moments (M2 = true): a simplex with vertices v_0..v_n, vertex sum s and volume |D| has the integral of
// theta theta^T = |D| / ((n + 1)(n + 2)) (sum_i v_i v_i^T + s s^T).  The M2 walk is the walk above with one more sum per wave: the packed
// upper triangle of sum |det| (sum_i v_i v_i^T + s s^T), n (n + 1) / 2 entries, entry e = lane + 64 u in accumulator u of its lane.  The
// Gram sum of the chain comes from LDS: at NT = 4 and 8 a chain Gs[k] = sum_{i<=k} a_i a_i^T pushed with the apex like Cs[k]; at NT = 16
// that chain would take 18.5 KB, so the chain's vertices Vx[k] are kept (2 KB) and the leaf adds their products.  The wave writes the
// entries to slot_m2 of its row; k_volume_reduce<true> has one thread per (polytope, entry), adds the slots in row order and writes the
// symmetric matrix.  Volume, centroid, count and status of the M2 pass are the additions of the volume pass: the same bits.
#pragma once
#include <stdint.h>

namespace mpc {

constexpr int VOL_MAX_ROWS = 256, VOL_MAX_VERTS = 16384, VOL_BATCH = 256, VOL_ROWSET_BLOCK = 256;
constexpr int VOL_OK = 0, VOL_UNBOUNDED = 1, VOL_NOT_POINTED = 2, VOL_EMPTY = 3, VOL_OVERFLOW = 4, VOL_TOO_LARGE = 5, VOL_INCONSISTENT = 6;

struct VolArgs {
    int nt;
    int c_in_lds;                      // the polytope's Ct are copied behind the stack in LDS
    long long n_items;
    const int32_t *item_q, *item_row;  // [n_items]: the polytope (index into chunk_poly) and the row of a wave
    const int32_t *chunk_poly;         // [chunk]: the polytope's index in the batch
    const long long *row_off, *vert_off;
    const double *vert;                // [vertices][nt]
    const unsigned long long *ct;      // Ct of the chunk's polytopes
    const long long *ct_off;           // [chunk]: words before polytope q's Ct
    long long max_simplices;
    unsigned long long *poly_count;    // [chunk]
    double *slot_vol, *slot_mom;       // [rows], [rows][nt]
    long long *slot_cnt;               // [rows]
    int32_t *slot_st;                  // [rows]
    double *slot_m2;                   // [rows][nt (nt + 1) / 2], M2 only
};

// entry e of the packed upper triangle of an n x n matrix (row major, i <= j): i | j << 4
__device__ inline int vol_tri_ij(int n, int e) {
    int i = 0;
    while (e >= n - i) { e -= n - i; ++i; }
    return i | (i + e) << 4;
}

__device__ inline int vol_wave_min(int v) {
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}
__device__ inline int vol_wave_max(int v) {
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}
__device__ inline int vol_wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ void __launch_bounds__(VOL_ROWSET_BLOCK) k_volume_rowsets(const int32_t *chunk_poly, const long long *row_off, const long long *vert_off,
                                                                     const unsigned long long *inc, const long long *ct_off,
                                                                     unsigned long long *ct) {
    const long long q = blockIdx.x, p = chunk_poly[q];
    const int m = (int)(row_off[p + 1] - row_off[p]);
    const long long v0 = vert_off[p], nv = vert_off[p + 1] - v0;
    const int W = (int)((nv + 63) / 64);
    unsigned long long *C = ct + ct_off[q];
    for (int idx = threadIdx.x; idx < W * m; idx += VOL_ROWSET_BLOCK) {
        const int w = idx / m, r = idx % m;
        const int hi = (int)min(64ll, nv - 64ll * w);
        unsigned long long bits = 0ull;
        for (int j = 0; j < hi; ++j) bits |= ((inc[(v0 + 64ll * w + j) * 4 + (r >> 6)] >> (r & 63)) & 1ull) << j;
        C[idx] = bits;
    }
}

template <int NT, bool M2>
__global__ void __launch_bounds__(64) k_volume_walk(VolArgs a) {
    constexpr bool GRAM = M2 && NT <= 8;              // the Gram chain in LDS; otherwise (M2) the chain's vertices
    constexpr int NTRI = NT * (NT + 1) / 2, NE = M2 ? (NTRI + 63) / 64 : 0;
    extern __shared__ unsigned long long vol_dyn[];   // stack [nt][W], then Ct [W][m] when c_in_lds
    __shared__ double Rr[NT + 1][NT];                 // row k of the eliminated chain (k = 1..nt)
    __shared__ double Cs[NT + 1][NT];                 // a_0 + ... + a_k
    __shared__ double Pr[NT + 1];                     // |pivot_1 ... pivot_k|
    __shared__ int Pc[NT + 1];                        // pivot column of row k
    __shared__ unsigned Um[NT + 1];                   // pivot columns of rows 1..k
    __shared__ unsigned long long Cand[NT + 1][4];    // rows still to try at level t
    __shared__ int Found[NT + 1];
    __shared__ double Gs[GRAM ? NT + 1 : 1][GRAM ? NTRI : 1];             // packed a_0 a_0^T + ... + a_k a_k^T
    __shared__ double Vx[M2 && !GRAM ? NT + 1 : 1][M2 && !GRAM ? NT : 1];  // a_k
    const int lane = threadIdx.x, nt = a.nt;
    const long long item = blockIdx.x;
    const int q = a.item_q[item], r_top = a.item_row[item];
    const long long p = a.chunk_poly[q];
    const int m = (int)(a.row_off[p + 1] - a.row_off[p]);
    const long long slot = a.row_off[p] + r_top;
    const long long v0 = a.vert_off[p];
    const int nv = (int)(a.vert_off[p + 1] - v0), W = (nv + 63) / 64;
    const double *X = a.vert + v0 * nt;
    const unsigned long long *C = a.ct + a.ct_off[q];
    unsigned long long *St = vol_dyn;
    if (a.c_in_lds) {
        unsigned long long *Cl = vol_dyn + nt * W;
        for (int i = lane; i < W * m; i += 64) Cl[i] = C[i];
        C = Cl;
    }
    for (int w = lane; w < W; w += 64) St[w] = (w == W - 1 && (nv & 63)) ? (1ull << (nv & 63)) - 1ull : ~0ull;
    if (lane < nt) Cs[0][lane] = X[lane];
    if (lane == 0) { Pr[0] = 1.0; Um[0] = 0u; }
    const int ne = nt * (nt + 1) / 2;
    double acc_m2[NE > 0 ? NE : 1];        // entry lane + 64 u of the packed triangle
    int eij[NE > 0 ? NE : 1];
    if constexpr (M2) {
#pragma unroll
        for (int u = 0; u < NE; ++u) {
            const int e = lane + 64 * u;
            acc_m2[u] = 0.0;
            eij[u] = e < ne ? vol_tri_ij(nt, e) : 0;
            if constexpr (GRAM) { if (e < ne) Gs[0][e] = X[eij[u] & 15] * X[eij[u] >> 4]; }
        }
        if constexpr (!GRAM) { if (lane < nt) Vx[0][lane] = X[lane]; }
    }
    __syncthreads();

    double acc_vol = 0.0, acc_mom = 0.0;   // acc_mom: coordinate `lane`
    long long count = 0;
    int status = VOL_OK;

    // x = vertex v - vertex 0, eliminated against rows 1..k-1 (lane c: coordinate c)
    auto eliminate = [&](int k, int v) {
        double x = lane < nt ? X[(long long)v * nt + lane] - X[lane] : 0.0;
        for (int j = 1; j < k; ++j) {
            const int pc = Pc[j];
            const double xp = __shfl(x, pc), pv = Rr[j][pc];
            const double f = pv != 0.0 ? xp / pv : 0.0;
            if (lane < nt) x -= f * Rr[j][lane];
            if (lane == pc) x = 0.0;
        }
        return x;
    };
    // the pivot of x among the columns not used by rows 1..k-1: largest magnitude, ties to the lowest column
    auto pivot_of = [&](int k, double x, int &pc) {
        const unsigned used = Um[k - 1];
        double best = (lane < nt && !((used >> lane) & 1u)) ? fabs(x) : -1.0;
        int bi = lane;
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best, off);
            const int oi = __shfl_xor(bi, off);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        pc = bi;
        return __shfl(x, bi);
    };
    // vertex v closes a simplex with the chain a_0..a_{nt-1}
    auto leaf = [&](int v) {
        int pc;
        const double x = eliminate(nt, v);
        const double vol = Pr[nt - 1] * fabs(pivot_of(nt, x, pc));
        acc_vol += vol;
        if (lane < nt) acc_mom += vol * (Cs[nt - 1][lane] + X[(long long)v * nt + lane]);
        if constexpr (M2) {
#pragma unroll
            for (int u = 0; u < NE; ++u) {
                const int e = lane + 64 * u, i = eij[u] & 15, j = eij[u] >> 4;
                if (e < ne) {
                    const double vi = X[(long long)v * nt + i], vj = X[(long long)v * nt + j];
                    double g = vi * vj + (Cs[nt - 1][i] + vi) * (Cs[nt - 1][j] + vj);
                    if constexpr (GRAM) g += Gs[nt - 1][e];
                    else for (int k = 0; k < nt; ++k) g += Vx[k][i] * Vx[k][j];
                    acc_m2[u] += vol * g;
                }
            }
        }
        ++count;
        if ((count & (VOL_BATCH - 1)) == 0) {
            unsigned long long tot = 0ull;
            if (lane == 0) tot = atomicAdd(&a.poly_count[q], (unsigned long long)VOL_BATCH) + VOL_BATCH;
            tot = __shfl(tot, 0);
            if ((long long)tot > a.max_simplices) status = VOL_TOO_LARGE;
        }
        if (count > a.max_simplices) status = VOL_TOO_LARGE;
    };
    // C_r avoids vertex `apex` of S, S & C_r is not empty, no other proper S & C_r' contains it strictly and none of a lower row equals it
    auto is_facet = [&](const unsigned long long *S, int r, int apex) {
        if ((C[(apex >> 6) * m + r] >> (apex & 63)) & 1ull) return false;
        bool reject = false, some = false;
        for (int r2 = lane; r2 < ((m + 63) & ~63); r2 += 64) {
            unsigned long long out = 0ull, rest = 0ull, more = 0ull, any = 0ull;
            if (r2 < m)
                for (int w = 0; w < W; ++w) {
                    const unsigned long long s = S[w], t = s & C[w * m + r], t2 = s & C[w * m + r2];
                    out |= t & ~t2; rest |= s & ~t2; more |= t2 & ~t; any |= t;
                }
            some = some || any != 0ull;
            reject = reject || (r2 < m && r2 != r && out == 0ull && rest != 0ull && (more != 0ull || r2 < r));
        }
        return __any(some) && !__any(reject);
    };
    auto write_slot = [&]() {
        if (lane == 0) { a.slot_vol[slot] = acc_vol; a.slot_cnt[slot] = count; a.slot_st[slot] = status; }
        if (lane < nt) a.slot_mom[slot * nt + lane] = acc_mom;
        if constexpr (M2) {
#pragma unroll
            for (int u = 0; u < NE; ++u) if (lane + 64 * u < ne) a.slot_m2[slot * ne + lane + 64 * u] = acc_m2[u];
        }
    };

    if (!is_facet(St, r_top, 0)) { write_slot(); return; }
    if (nt == 1) {
        // an interval: the facet is its other end
        int cnt = 0, hi = -1;
        for (int w = lane; w < W; w += 64) { const unsigned long long t = C[w * m + r_top]; cnt += __popcll(t); if (t) hi = w * 64 + 63 - __clzll(t); }
        cnt = vol_wave_sum(cnt); hi = vol_wave_max(hi);
        if (cnt != 1) status = VOL_INCONSISTENT; else leaf(hi);
        write_slot();
        return;
    }
    for (int w = lane; w < W; w += 64) St[W + w] = St[w] & C[w * m + r_top];
    __syncthreads();
    int t = 1;
    bool enter = true;
    while (t >= 1 && status == VOL_OK) {
        unsigned long long *S = St + t * W;
        if (enter) {
            // the face S of dimension nt - t: its apex joins the chain as row t
            int lo = 0x7fffffff, hi = -1, cnt = 0;
            for (int w = lane; w < W; w += 64) {
                const unsigned long long s = S[w];
                if (s) { lo = min(lo, w * 64 + __ffsll((long long)s) - 1); hi = w * 64 + 63 - __clzll(s); }
                cnt += __popcll(s);
            }
            const int apex = vol_wave_min(lo);
            int pc;
            const double x = eliminate(t, apex);
            const double pv = pivot_of(t, x, pc);
            __syncthreads();
            if (lane < nt) { Rr[t][lane] = x; Cs[t][lane] = Cs[t - 1][lane] + X[(long long)apex * nt + lane]; }
            if (lane == 0) { Pc[t] = pc; Um[t] = Um[t - 1] | 1u << pc; Pr[t] = Pr[t - 1] * fabs(pv); Found[t] = 0; }
            if constexpr (GRAM) {
                if (lane < ne) Gs[t][lane] = Gs[t - 1][lane] + X[(long long)apex * nt + (eij[0] & 15)] * X[(long long)apex * nt + (eij[0] >> 4)];
            } else if constexpr (M2) {
                if (lane < nt) Vx[t][lane] = X[(long long)apex * nt + lane];
            }
            __syncthreads();
            if (t == nt - 1) {
                // an edge: its facet without the apex is its other vertex
                if (vol_wave_sum(cnt) != 2) status = VOL_INCONSISTENT; else leaf(vol_wave_max(hi));
                --t; enter = false;
                continue;
            }
            for (int g = 0; g < 4; ++g) {
                const int r = g * 64 + lane;
                bool cand = false;
                if (r < m && !((C[(apex >> 6) * m + r] >> (apex & 63)) & 1ull))
                    for (int w = 0; w < W && !cand; ++w) cand = (S[w] & C[w * m + r]) != 0ull;
                const unsigned long long mask = __ballot(cand);
                if (lane == 0) Cand[t][g] = mask;
            }
            __syncthreads();
            enter = false;
        }
        // the next candidate row of level t
        int r = -1;
        for (int g = 0; g < 4 && r < 0; ++g) { const unsigned long long c = Cand[t][g]; if (c) r = g * 64 + __ffsll((long long)c) - 1; }
        if (r < 0) {
            if (!Found[t]) status = VOL_INCONSISTENT;
            --t;
            continue;
        }
        __syncthreads();
        if (lane == 0) Cand[t][r >> 6] &= ~(1ull << (r & 63));
        int lo = 0x7fffffff;
        for (int w = lane; w < W; w += 64) { const unsigned long long s = S[w]; if (s) lo = min(lo, w * 64 + __ffsll((long long)s) - 1); }
        const int apex = vol_wave_min(lo);
        const bool facet = is_facet(S, r, apex);
        if (facet) {
            if (lane == 0) Found[t] = 1;
            for (int w = lane; w < W; w += 64) S[W + w] = S[w] & C[w * m + r];
            ++t; enter = true;
        }
        __syncthreads();
    }
    write_slot();
}

// adds the slots of every polytope of a chunk in row order and scales: volume = sum / n!, centroid = moment / ((n + 1) sum).  M2: the grid
// has one row of blocks per entry of the packed triangle; a thread adds that entry too, second moment = sum / (n! (n + 1)(n + 2)), and
// the threads of entry 0 write what the volume pass writes
template <bool M2>
__global__ void __launch_bounds__(64) k_volume_reduce(int nt, long long n, const int32_t *chunk_poly, const long long *row_off, long long max_simplices,
                                                      const double *slot_vol, const double *slot_mom, const long long *slot_cnt,
                                                      const int32_t *slot_st, const double *slot_m2, double *volume, double *centroid,
                                                      long long *n_simplices, int32_t *status, double *second_moment) {
    const long long q = (long long)blockIdx.x * 64 + threadIdx.x;
    if (q >= n) return;
    const long long p = chunk_poly[q];
    const bool lead = !M2 || blockIdx.y == 0;
    const int e = M2 ? (int)blockIdx.y : 0, ne = nt * (nt + 1) / 2;
    double vol = 0.0, mom[16], m2 = 0.0;
    for (int c = 0; c < 16; ++c) mom[c] = 0.0;
    long long cnt = 0;
    bool large = false, bad = false;
    for (long long s = row_off[p]; s < row_off[p + 1]; ++s) {
        vol += slot_vol[s];
        cnt += slot_cnt[s];
        large = large || slot_st[s] == VOL_TOO_LARGE;
        bad = bad || slot_st[s] == VOL_INCONSISTENT;
        if constexpr (M2) m2 += slot_m2[s * ne + e];
        if (lead) {
#pragma unroll
            for (int c = 0; c < 16; ++c) if (c < nt) mom[c] += slot_mom[s * nt + c];
        }
    }
    const int st = (large || cnt > max_simplices) ? VOL_TOO_LARGE : (bad || cnt == 0) ? VOL_INCONSISTENT : VOL_OK;
    double fact = 1.0;
    for (int k = 2; k <= nt; ++k) fact *= k;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (lead) {
        status[p] = st;
        n_simplices[p] = st == VOL_OK ? cnt : 0;
        volume[p] = st == VOL_OK ? vol / fact : nan;
#pragma unroll
        for (int c = 0; c < 16; ++c) if (c < nt) centroid[p * nt + c] = st == VOL_OK ? mom[c] / ((nt + 1) * vol) : nan;
    }
    if constexpr (M2) {
        const int ij = vol_tri_ij(nt, e), i = ij & 15, j = ij >> 4;
        const double v = st == VOL_OK ? m2 / (fact * ((nt + 1) * (nt + 2))) : nan;
        second_moment[(p * nt + i) * nt + j] = v;
        second_moment[(p * nt + j) * nt + i] = v;
    }
}

}  // namespace mpc
