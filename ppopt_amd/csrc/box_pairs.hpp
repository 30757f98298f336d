// box_pairs.hpp -- the candidate sweep of Solution.compare, transition_graph and remove_overlaps on the device (gfx950), and the row
// screen behind it; DESIGN §3.27.
//
// Boxes arrive as [R][2][n_t] (lower bounds, then upper bounds) with one usable byte per box.  A NaN lower bound reads as -inf, a NaN
// upper bound as +inf.  The pair (i, j) of a box of family a and a box of family b is listed iff both are usable and for every
// coordinate k
//                         min(hi_a[i][k], hi_b[j][k]) - max(lo_a[i][k], lo_b[j][k]) > margin
// in fp64: one subtraction and a strict compare, infinities as ordinary values, an inf - inf that gives NaN fails.  BP_CROSS lists every
// (i, j), i = j included; BP_UPPER takes one family against itself and lists i < j only.
//
//   k_box_pairs<NT, EMIT>  NT in {4, 8, 16}.  One LANE owns one a-box, its 2 NT bounds in registers (coordinates past n_t: -inf / +inf,
//                          which pass).  A workgroup of BP_BLOCK lanes stages BP_TILE b-boxes in LDS as structure of arrays
//                          (s_lo[k][jj], s_hi[k][jj]); in the test loop every lane reads the same address, a broadcast.  An unusable
//                          b-box, and the tail of the last tile, is staged as lo = +inf, hi = -inf: -inf - +inf = -inf fails in
//                          coordinate 0 whatever the a-box holds, so the loop has no usable test.  The grid is (row blocks, segments):
//                          segment s covers seg_tiles consecutive tiles of family b.
//       EMIT = false       counts[row][segment] = the hits of that lane in that segment.
//       (host)             an exclusive scan of counts in (row, segment) order: offsets, and the total behind the last entry.
//       EMIT = true        the same tests again; the lane writes its hits from offsets[row][segment] on, in ascending j.
//                          The list is ascending by (i, j) by construction; no atomic anywhere, a rerun gives the same bytes.
//   k_box_row_counts       row_count[r] = offsets[r + 1][0] - offsets[r][0].
//   k_pair_screen<NT>      one lane per candidate (i, j).  Side A: the rows of region i against box_for_a[j]; side B: the rows of
//                          region j against box_for_b[i].  For a unit row [o | n], s = sum over ascending k of n_k (lo[k] if n_k > 0
//                          else hi[k]), terms with n_k == 0 skipped, is the least n.theta on the box; the row separates when
//                          s - o > PS_EPS (1 + |o|), and the pair is dropped at the first row that does.  A NaN s separates nothing.
//                          Rows come from global memory (L2); candidates are sorted by i, so the lanes of a wavefront mostly read the
//                          same rows on side A.  The only atomics are the three counters, one add per wavefront.
#pragma once
#include <stdint.h>

namespace mpc {

constexpr int BP_BLOCK = 256, BP_TILE = 128, BP_MAX_SEG = 64, BP_MAX_NT = 16;
constexpr double PS_EPS = 1e-12;
enum { BP_CROSS = 0, BP_UPPER = 1 };
enum { PS_SIDE_A = 1, PS_SIDE_B = 2 };

struct BoxPairArgs {
    int nt, mode, n_seg, seg_tiles;
    long long n_b, n_tiles, i0, rows;       // the rows [i0, i0 + rows) of family a
    const double *box_a, *box_b;
    const uint8_t *usable_a, *usable_b;
    double margin;
    unsigned long long *counts;             // [rows][n_seg], written by the count pass
    const unsigned long long *offsets;      // [rows][n_seg], read by the emit pass
    long long *pair_a, *pair_b;             // [total], written by the emit pass
};

template <int NT, bool EMIT> __global__ void __launch_bounds__(BP_BLOCK) k_box_pairs(BoxPairArgs a) {
    __shared__ double s_lo[NT][BP_TILE], s_hi[NT][BP_TILE];
    const int tid = threadIdx.x, nt = a.nt;
    const long long r = (long long)blockIdx.x * BP_BLOCK + tid, i = a.i0 + r, seg = blockIdx.y;
    const bool in_range = r < a.rows, live = in_range && a.usable_a[i] != 0;
    double lo[NT], hi[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        double l = -INFINITY, h = INFINITY;
        if (live && k < nt) {
            l = a.box_a[(2 * i) * nt + k];
            h = a.box_a[(2 * i + 1) * nt + k];
            l = isnan(l) ? -INFINITY : l;
            h = isnan(h) ? INFINITY : h;
        }
        lo[k] = l;
        hi[k] = h;
    }
    // the coordinates past n_t are open in every tile; the staging below never touches them
    for (int e = tid; e < (NT - nt) * BP_TILE; e += BP_BLOCK) {
        s_lo[nt + e / BP_TILE][e % BP_TILE] = -INFINITY;
        s_hi[nt + e / BP_TILE][e % BP_TILE] = INFINITY;
    }
    const long long tile0 = seg * a.seg_tiles, tile1 = tile0 + a.seg_tiles < a.n_tiles ? tile0 + a.seg_tiles : a.n_tiles;
    const long long i_min = a.i0 + (long long)blockIdx.x * BP_BLOCK;      // the smallest i of this workgroup
    unsigned long long n = 0;
    long long pos = 0;
    if (EMIT && in_range) pos = (long long)a.offsets[r * a.n_seg + seg];
    for (long long tile = tile0; tile < tile1; ++tile) {
        const long long j0 = tile * BP_TILE;
        if (a.mode == BP_UPPER && j0 + BP_TILE <= i_min + 1) continue;    // every j of the tile is <= every i here (uniform: no lane waits)
        const int cnt = a.n_b - j0 < BP_TILE ? (int)(a.n_b - j0) : BP_TILE;
        __syncthreads();
        for (int e = tid; e < BP_TILE * 2 * nt; e += BP_BLOCK) {
            const int jj = e / (2 * nt), rem = e - jj * 2 * nt, side = rem / nt, k = rem - side * nt;
            const bool ok = jj < cnt && a.usable_b[j0 + jj] != 0;
            double v = 0.0;
            if (ok) v = a.box_b[j0 * 2 * nt + e];
            if (side == 0) s_lo[k][jj] = ok ? (isnan(v) ? -INFINITY : v) : INFINITY;
            else s_hi[k][jj] = ok ? (isnan(v) ? INFINITY : v) : -INFINITY;
        }
        __syncthreads();
        if (live) {
            for (int jj = 0; jj < cnt; ++jj) {
                bool hit = a.mode != BP_UPPER || j0 + jj > i;
#pragma unroll
                for (int k = 0; k < NT; ++k) hit = hit & (fmin(hi[k], s_hi[k][jj]) - fmax(lo[k], s_lo[k][jj]) > a.margin);
                if (hit) {
                    if (EMIT) {
                        a.pair_a[pos] = i;
                        a.pair_b[pos] = j0 + jj;
                        ++pos;
                    }
                    ++n;
                }
            }
        }
    }
    if (!EMIT && in_range) a.counts[r * a.n_seg + seg] = n;
}

__global__ void __launch_bounds__(256) k_box_row_counts(long long rows, int n_seg, const unsigned long long *__restrict__ offsets,
                                                        long long *__restrict__ row_count) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r < rows) row_count[r] = (long long)(offsets[(r + 1) * n_seg] - offsets[r * n_seg]);
}

struct PairScreenArgs {
    int nt, sides;
    long long n_pairs;
    const long long *row_off;
    const double *ef;                        // [rows][nt + 1] unit [o | n]
    const long long *pair_a, *pair_b;
    const double *box_for_a, *box_for_b;     // [n_regions][2][nt]; the one of a side that is not screened may be nullptr
    uint8_t *keep;
    unsigned long long *counters;            // pairs, dropped, rows read
};

template <int NT> __global__ void __launch_bounds__(256) k_pair_screen(PairScreenArgs a) {
    const int nt = a.nt, nr = nt + 1;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = q < a.n_pairs;
    unsigned long long rows_read = 0, pairs = live ? 1 : 0, dropped = 0;
    if (live) {
        const long long pi = a.pair_a[q], pj = a.pair_b[q];
        bool keep = true;
        for (int side = 0; side < 2 && keep; ++side) {
            if (!(a.sides >> side & 1)) continue;
            const long long reg = side ? pj : pi, other = side ? pi : pj;
            const double *box = (side ? a.box_for_b : a.box_for_a) + 2 * other * nt;
            double lo[NT], hi[NT];
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                lo[k] = k < nt ? box[k] : 0.0;
                hi[k] = k < nt ? box[nt + k] : 0.0;
            }
            const long long r1 = a.row_off[reg + 1];
            for (long long rr = a.row_off[reg]; rr < r1 && keep; ++rr) {
                const double *row = a.ef + rr * nr;
                const double o = row[0];
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    if (k < nt) {
                        const double v = row[1 + k];
                        if (v > 0.0) s = s + v * lo[k];
                        else if (v < 0.0) s = s + v * hi[k];
                    }
                }
                ++rows_read;
                keep = !(s - o > PS_EPS * (1.0 + fabs(o)));
            }
        }
        a.keep[q] = keep ? 1 : 0;
        dropped = keep ? 0 : 1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        rows_read += __shfl_down(rows_read, off);
        pairs += __shfl_down(pairs, off);
        dropped += __shfl_down(dropped, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(a.counters + 0, pairs);
        atomicAdd(a.counters + 1, dropped);
        atomicAdd(a.counters + 2, rows_read);
    }
}

}  // namespace mpc
