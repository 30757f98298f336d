// locate.hpp -- point location over the critical regions of a Solution, and evaluation of x*(theta), batched (gfx950).
//
// Reference: Solution.get_region / evaluate (solution.py:45-112): a loop over the regions calling
// CriticalRegion.is_inside, all(E theta - f < tol) (critical_region.py:83-86); without overlap the first region of the list
// that contains theta wins, with overlap the containing region with the lowest objective (ties: the later one).
//
// Mapping: one LANE per query point, the wavefront walks the region list.  Region and row indices are wave-uniform, so a
// row [f | E] is fetched with scalar loads and applied to 64 points at once; no gathers, no divergence except the exit
// masks.  A region is left as soon as no lane of the wave is still inside it, the list as soon as every lane has its
// region (first-match mode).  The stacked rows (13.7 MB for the 9,432 regions of config 4) stay in L2 / Infinity Cache.
#pragma once
#include <stdint.h>

namespace mpc {

// The scan's membership test of one row [f | E] and its objective of a region's law; shared with k_locate_tree (tree.hpp), so that both
// locators form the same numbers with the same operations.
//   inclusive: E theta <= f + tol with the product formed first and then compared, like `A @ theta <= b` of the reference's
//   PointLocation (upop/point_location.py:46,59): a point exactly on a facet belongs to the region;  strict: E theta - f < tol.
template <int NT>
__device__ __forceinline__ bool loc_row_inside(const double *row, const double (&th)[NT], int nt, double tol, int inclusive) {
    if (inclusive) {
        double v = 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) if (t < nt) v = fma(row[1 + t], th[t], v);
        return v <= row[0] + tol;
    }
    double v = -row[0];
#pragma unroll
    for (int t = 0; t < NT; ++t) if (t < nt) v = fma(row[1 + t], th[t], v);
    return v < tol;
}

// objective 1/2 x'Qx + theta'H'x + c'x at x = A theta + b (terms without x are the same for every region); xl = [b | A] of the region
template <int NT>
__device__ __forceinline__ double loc_objective(const double *xl, int nx, int nt, const double (&th)[NT], const double *cvec, const double *H,
                                                const double *Q) {
    const int nr = nt + 1;
    double obj = 0.0;
    for (int a = 0; a < nx; ++a) {
        double xa = xl[a * nr];
#pragma unroll
        for (int t = 0; t < NT; ++t) if (t < nt) xa = fma(xl[a * nr + 1 + t], th[t], xa);
        double g = cvec ? cvec[a] : 0.0;
        if (H) {
#pragma unroll
            for (int t = 0; t < NT; ++t) if (t < nt) g = fma(H[a * nt + t], th[t], g);
        }
        if (Q) {
            double qx = 0.0;
            for (int j = 0; j < nx; ++j) {
                double xj = xl[j * nr];
#pragma unroll
                for (int t = 0; t < NT; ++t) if (t < nt) xj = fma(xl[j * nr + 1 + t], th[t], xj);
                qx = fma(Q[a * nx + j], xj, qx);
            }
            g = fma(0.5, qx, g);
        }
        obj = fma(g, xa, obj);
    }
    return obj;
}

// Rows are staged through LDS in tiles of LOC_TILE rows, loaded cooperatively (coalesced) by the 256 points of a block;
// with each row come the region it belongs to and the index of the first row of the next region, so that a wavefront
// which has no lane left inside a region jumps over the rest of its rows.
constexpr int LOC_TILE = 256;

// The scan of one point per lane, shared by k_locate and k_simulate (closed_loop.hpp).  Every thread of the block calls it (it stages
// the rows with barriers); `active` is false for a lane without a point, which only helps to stage.  tile / trid / tend: LDS of
// LOC_TILE rows.  Returns the region (-1: none).
template <int NT>
__device__ __forceinline__ long long loc_scan_block(bool active, const double (&th)[NT], int nt, int nx, long long n_rows,
                                                    const int32_t *__restrict__ row_region, const int32_t *__restrict__ row_end,
                                                    const double *__restrict__ ef, const double *__restrict__ xlaw, const double *__restrict__ Q,
                                                    const double *__restrict__ cvec, const double *__restrict__ H, double tol, int overlapping,
                                                    int inclusive, double (*tile)[NT + 1], int *trid, int *tend) {
    const int nr = nt + 1;
    long long found = -1;
    double best = INFINITY;
    bool alive = active, inside = false;
    int cur = -1;
    long long i = 0;   // next row of this wavefront (wave-uniform)
    // the point is inside every row of region `cur`: first match, or candidate for the lowest objective
    auto commit = [&]() {
        if (cur < 0 || !inside) return;
        if (!overlapping) { found = cur; alive = false; return; }
        const double obj = loc_objective<NT>(xlaw + (size_t)cur * nx * nr, nx, nt, th, cvec, H, Q);
        if (obj <= best) { best = obj; found = cur; }
    };
    for (long long tile0 = 0; tile0 < n_rows; tile0 += LOC_TILE) {
        __syncthreads();
        {
            const long long row = tile0 + threadIdx.x;
            if (row < n_rows) {
#pragma unroll
                for (int t = 0; t <= NT; ++t) tile[threadIdx.x][t] = t <= nt ? ef[row * nr + t] : 0.0;
                trid[threadIdx.x] = row_region[row];
                tend[threadIdx.x] = row_end[row];
            }
        }
        __syncthreads();
        const long long tile1 = tile0 + LOC_TILE < n_rows ? tile0 + LOC_TILE : n_rows;
        while (i < tile1) {
            const int li = (int)(i - tile0);
            const int rid = trid[li];
            if (rid != cur) {
                commit();
                cur = rid;
                inside = overlapping ? active : alive;
                if (!overlapping && !__any(alive)) { i = n_rows; break; }   // every lane has its region
            }
            inside = inside && loc_row_inside<NT>(tile[li], th, NT, tol, inclusive);   // tile rows are zero past nt
            if (!__any(inside)) { i = tend[li]; continue; }   // nobody is left in this region: on to the next one
            ++i;
        }
    }
    commit();
    return found;
}

template <int NT>
__global__ void __launch_bounds__(256) k_locate(long long m, int nt, int nx, long long n_regions, long long n_rows,
                                                const int32_t *__restrict__ row_region, const int32_t *__restrict__ row_end,
                                                const double *__restrict__ ef, const double *__restrict__ xlaw,
                                                const double *__restrict__ Q, const double *__restrict__ cvec, const double *__restrict__ H,
                                                const double *__restrict__ theta, double tol, int overlapping, int inclusive,
                                                long long *__restrict__ region_out) {
    __shared__ double tile[LOC_TILE][NT + 1];
    __shared__ int trid[LOC_TILE], tend[LOC_TILE];
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double th[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) th[t] = (p < m && t < nt) ? theta[p * nt + t] : 0.0;
    const long long found = loc_scan_block<NT>(p < m, th, nt, nx, n_rows, row_region, row_end, ef, xlaw, Q, cvec, H, tol, overlapping, inclusive,
                                               tile, trid, tend);
    if (p < m) region_out[p] = found;
}

// The list scan of one lane on its own (no barriers, no LDS): the fallback of k_simulate for a point the walk or the tree left
// unresolved.  The scan's row test and objective, regions in list order: the first containing region, or with `overlapping` the
// containing region of lowest objective, ties to the later one -- the answer of loc_scan_block.
template <int NT>
__device__ __forceinline__ long long loc_scan_lane(const double (&th)[NT], int nt, int nx, long long n_regions, const long long *__restrict__ row_off,
                                                   const double *__restrict__ ef, const double *__restrict__ xlaw, const double *__restrict__ Q,
                                                   const double *__restrict__ cvec, const double *__restrict__ H, double tol, int overlapping,
                                                   int inclusive) {
    const int nr = nt + 1;
    long long found = -1;
    double best = INFINITY;
    for (long long r = 0; r < n_regions; ++r) {
        if (row_off[r + 1] <= row_off[r]) continue;   // the scan walks rows: a region without rows is never met
        bool inside = true;
        for (long long k = row_off[r]; k < row_off[r + 1] && inside; ++k) inside = loc_row_inside<NT>(ef + k * nr, th, nt, tol, inclusive);
        if (!inside) continue;
        if (!overlapping) return r;
        const double obj = loc_objective<NT>(xlaw + (size_t)r * nx * nr, nx, nt, th, cvec, H, Q);
        if (obj <= best) { best = obj; found = r; }
    }
    return found;
}

// ------------------------------------------------------------------------------------------------------------------
// k_locate_walk: point location by walking through ADJACENT regions (complete, non-overlapping solutions with many regions).
//
// The list scan above costs every point a pass over all rows of all regions it is not in -- 4.1e6 rows for the 227,349
// regions of the complete config 4.  The regions of an mpQP solution are glued along their facets, and a facet knows what
// lies behind it: the row of a multiplier lambda_a >= 0 is shared with the region whose active set lacks a, the row of an
// inactive constraint c with the region whose active set has c in addition (Bemporad et al. 2002; the reference's graph
// algorithm moves the same way, mpqp_graph.py:97-106), a row of A_t theta <= b_t with nothing.  One lane per point: test the
// rows of the current region; if all hold the point is located, otherwise cross the most violated row to the neighbour, whose
// region index comes from a binary search of its active-set mask in the sorted mask table.  A point that meets a row of the
// parameter set is outside the solution (-1); a walk that finds no neighbour behind any violated row (not even with a second
// row exchanged, the degenerate case), meets a region without facet information or reaches the step limit leaves the point
// UNRESOLVED (-2), and the host hands it to k_locate_few / the list scan.
// To return the region the scan would return (the FIRST containing region of the list), the located region is certified by the
// 2*tol rule: a point that satisfies every row by 2*tol or more is taken to lie in no other region within tol.  With exactly ONE row
// nearer than that, the only other candidate is taken to be the neighbour across it, which wins if it comes earlier in the list and
// contains the point within tol; if that neighbour is unknown the point is left unresolved.  With TWO OR MORE near rows the point
// is next to a face of codimension >= 2, where regions that are no neighbours across a row (diagonally across a corner) may contain
// it too: unresolved (-2) as well, and the exhaustive pass decides.  A row value that is not a number (NaN in theta) is never
// certified either.
// ASSUMPTION of the 2*tol rule: tol is applied to the row values as they are stored, so the rows of neighbouring regions have
// comparable scale (unit rows: the values are distances), and the facets that meet in a corner do so at a right or obtuse angle.  A
// region diagonally across a corner of acute wedge angle alpha holds points up to tol / sin(alpha / 2) from the corner, which exceeds
// 2 tol below 60 degrees: such a point can be 2 tol from both rows of the located region and still lie within tol in an earlier
// region, and the walk then returns the located one.  The same holds where one region's rows are scaled far below its neighbour's.
// Within the assumption the walk returns the scan's region; outside it, a region that contains the point within tol, not always
// the first of the list.
// row_info[row] = kind << 16 | id:  kind 0 multiplier row of active constraint id, 1 inactive constraint id, 2 A_t row, 3 unknown.
// The walk of one lane from start_region (shared by k_locate_walk and k_simulate): the region (-1 outside, -2 unresolved); `crossings`
// counts the regions crossed.
template <int NT, int MW>
__device__ __forceinline__ long long loc_walk(const double (&th)[NT], int nt, long long n_regions, const long long *__restrict__ row_off,
                                              const double *__restrict__ ef, const int32_t *__restrict__ row_info,
                                              const unsigned long long *__restrict__ masks,          // [n_regions][MW], region order
                                              const unsigned long long *__restrict__ sorted_masks,   // [n_regions][MW], ascending
                                              const int32_t *__restrict__ sorted_region,             // region of sorted_masks[i]
                                              double tol, long long start_region, int max_steps, int n_c, unsigned long long &crossings) {
    const int nr = nt + 1;
    auto lookup = [&](const unsigned long long (&key)[MW]) -> long long {
        long long lo = 0, hi = n_regions;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            bool less = false, decided = false;
#pragma unroll
            for (int j = MW - 1; j >= 0; --j) {
                const unsigned long long v = sorted_masks[mid * MW + j];
                if (!decided && v != key[j]) { less = v < key[j]; decided = true; }
            }
            if (less) lo = mid + 1; else hi = mid;
        }
        if (lo >= n_regions) return -1;
#pragma unroll
        for (int j = 0; j < MW; ++j) if (sorted_masks[lo * MW + j] != key[j]) return -1;
        return sorted_region[lo];
    };
    // worst row of region r at theta (value and row); returns false if the region has a row of unknown kind
    auto worst_row = [&](long long r, double &worst, long long &wrow) {
        worst = -INFINITY; wrow = -1;
        for (long long i = row_off[r]; i < row_off[r + 1]; ++i) {
            double v = -ef[i * nr];
#pragma unroll
            for (int t = 0; t < NT; ++t) if (t < nt) v = fma(ef[i * nr + 1 + t], th[t], v);
            if (v > worst) { worst = v; wrow = i; }
        }
    };
    auto neighbour = [&](long long r, long long row) -> long long {   // -1 outside, -2 unknown
        const int info = row_info[row], kind = info >> 16, id = info & 0xffff;
        if (kind == 2) return -1;
        if (kind == 3) return -2;
        unsigned long long key[MW];
#pragma unroll
        for (int j = 0; j < MW; ++j) key[j] = masks[r * MW + j];
#pragma unroll
        for (int j = 0; j < MW; ++j) if ((id >> 6) == j) key[j] ^= 1ull << (id & 63);
        const long long q = lookup(key);
        return q < 0 ? -2 : q;
    };
    long long r = start_region, prev = -1, found = -2;
    for (int step = 0; step < max_steps; ++step) {
        // the violated rows of region r in decreasing order of violation, until one has a region behind it.  (Redundancy removal
        // keeps rows that only touch the region in a lower-dimensional face -- mpqp_utils.py:143-178 keeps weakly redundant
        // rows -- and nothing lies behind those; a true facet of a complete solution has a neighbour unless it is part of the
        // boundary of the feasible parameter set.)
        double bound = INFINITY;
        long long next = -2;
        bool any_violated = false, met_omega = false, met_unknown = false;
        for (;;) {
            double worst = -INFINITY; long long wrow = -1;
            for (long long i = row_off[r]; i < row_off[r + 1]; ++i) {
                double v = -ef[i * nr];
#pragma unroll
                for (int t = 0; t < NT; ++t) if (t < nt) v = fma(ef[i * nr + 1 + t], th[t], v);
                if (v > worst && v < bound) { worst = v; wrow = i; }
            }
            if (wrow < 0 || worst < tol) break;          // no (further) violated row
            any_violated = true;
            const long long q = neighbour(r, wrow);
            if (q >= 0 && q != prev) { next = q; break; }   // never straight back: two regions that both see the point behind their common facet
            if (q == -1) { met_omega = true; if (worst > 10.0 * tol) break; }   // clearly outside the parameter set: no region can contain the point
            else if ((row_info[wrow] >> 16) >= 3) met_unknown = true;
            bound = worst;
        }
        if (!any_violated) { found = row_off[r + 1] > row_off[r] ? r : -2; break; }
        if (next >= 0) { prev = r; r = next; ++crossings; continue; }
        // Every violated row leads nowhere with one row added or removed.  Where the constraint gradients are dependent the
        // region behind a facet differs by TWO rows (one enters, one leaves): try, for the most violated rows, the neighbour's
        // active set with one further row exchanged, and take the first that exists and is violated less than this region.
        if (!met_omega) {
            double vbound = INFINITY;
            for (int attempt = 0; attempt < 3 && next < 0; ++attempt) {
                double worst = -INFINITY; long long wrow = -1;
                for (long long i = row_off[r]; i < row_off[r + 1]; ++i) {
                    double v = -ef[i * nr];
#pragma unroll
                    for (int t = 0; t < NT; ++t) if (t < nt) v = fma(ef[i * nr + 1 + t], th[t], v);
                    if (v > worst && v < vbound) { worst = v; wrow = i; }
                }
                if (wrow < 0 || worst < tol) break;
                vbound = worst;
                const int info = row_info[wrow], kind = info >> 16, id = info & 0xffff;
                if (kind >= 2) continue;
                unsigned long long base[MW];
#pragma unroll
                for (int j = 0; j < MW; ++j) base[j] = masks[r * MW + j];
#pragma unroll
                for (int j = 0; j < MW; ++j) if ((id >> 6) == j) base[j] ^= 1ull << (id & 63);
                for (int c2 = 0; c2 < n_c && next < 0; ++c2) {
                    if (c2 == id) continue;
                    const bool in_set = (base[c2 >> 6] >> (c2 & 63)) & 1ull;
                    if ((kind == 1) != in_set) continue;          // a row entered: one of the others leaves; a row left: another enters
                    unsigned long long key[MW];
#pragma unroll
                    for (int j = 0; j < MW; ++j) key[j] = base[j];
                    key[c2 >> 6] ^= 1ull << (c2 & 63);
                    const long long q = lookup(key);
                    if (q >= 0 && q != r) {
                        double w; long long wr;
                        worst_row(q, w, wr);
                        if (wr >= 0 && w < worst) next = q;       // strictly less violated: the walk cannot return here through this move
                    }
                }
            }
        }
        if (next >= 0) { prev = r; r = next; ++crossings; continue; }
        found = met_omega ? -1 : -2;
        break;
    }
    if (found >= 0) {
        // first-match rule of the list scan: certify the located region (see above)
        int near = 0;
        long long near_row = -1;
        for (long long i = row_off[found]; i < row_off[found + 1]; ++i) {
            double v = -ef[i * nr];
#pragma unroll
            for (int t = 0; t < NT; ++t) if (t < nt) v = fma(ef[i * nr + 1 + t], th[t], v);
            if (!(v < tol)) { near = 2; break; }   // NaN: not located at all
            if (v > -2.0 * tol) { ++near; near_row = i; }
        }
        if (near >= 2) found = -2;
        else if (near == 1) {
            const long long q = neighbour(found, near_row);
            if (q == -2) found = -2;               // what lies behind the near row is unknown
            else if (q >= 0 && q < found) {
                double w; long long wr;
                worst_row(q, w, wr);
                if (wr >= 0 && w < tol) found = q;
            }
        }
    }
    return found;
}

template <int NT, int MW>
__global__ void __launch_bounds__(256) k_locate_walk(long long m, int nt, long long n_regions, const long long *__restrict__ row_off,
                                                     const double *__restrict__ ef, const int32_t *__restrict__ row_info,
                                                     const unsigned long long *__restrict__ masks,          // [n_regions][MW], region order
                                                     const unsigned long long *__restrict__ sorted_masks,   // [n_regions][MW], ascending
                                                     const int32_t *__restrict__ sorted_region,             // region of sorted_masks[i]
                                                     const double *__restrict__ theta, double tol, int start_region, int max_steps,
                                                     int n_c, long long *__restrict__ region_out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    double th[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) th[t] = t < nt ? theta[p * nt + t] : 0.0;
    unsigned long long crossings = 0;
    region_out[p] = loc_walk<NT, MW>(th, nt, n_regions, row_off, ef, row_info, masks, sorted_masks, sorted_region, tol, start_region, max_steps,
                                     n_c, crossings);
}

// The few points the walk left unresolved: one thread per (point, region), the first containing region by atomicMin.
// Work = points x rows, spread over the whole device -- the list scan would serialise 4e6 rows behind one wavefront.
template <int NT>
__global__ void __launch_bounds__(256) k_locate_few(long long n_pts, int nt, long long n_regions, const long long *__restrict__ row_off,
                                                    const double *__restrict__ ef, const double *__restrict__ theta, double tol,
                                                    long long *__restrict__ region_out) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long p = blockIdx.y;
    if (r >= n_regions || p >= n_pts) return;
    const int nr = nt + 1;
    double th[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) th[t] = t < nt ? theta[p * nt + t] : 0.0;
    const long long i0 = row_off[r], i1 = row_off[r + 1];
    if (i1 <= i0) return;
    bool inside = true;
    for (long long i = i0; i < i1 && inside; ++i) {
        double v = -ef[i * nr];
#pragma unroll
        for (int t = 0; t < NT; ++t) if (t < nt) v = fma(ef[i * nr + 1 + t], th[t], v);
        inside = v < tol;
    }
    if (inside) atomicMin(reinterpret_cast<unsigned long long *>(region_out + p), (unsigned long long)r);
}

// x*(theta) = A theta + b of the region each point was located in (NaN where there is none)
__global__ void __launch_bounds__(256) k_evaluate(long long m, int nt, int nx, const double *__restrict__ xlaw, const double *__restrict__ theta,
                                                  const long long *__restrict__ region, double *__restrict__ x) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * nx) return;
    const long long p = idx / nx;
    const int i = (int)(idx - p * nx);
    const long long r = region[p];
    if (r < 0) { x[idx] = __longlong_as_double(0x7ff8000000000000ll); return; }
    const int nr = nt + 1;
    const double *row = xlaw + ((size_t)r * nx + i) * nr;
    double v = row[0];
    for (int t = 0; t < nt; ++t) v = fma(row[1 + t], theta[p * nt + t], v);
    x[idx] = v;
}


// ------------------------------------------------------------------------------------------------------------------
// k_hit_and_run: hit-and-run Markov chains in a batch of polytopes {x : A_p x <= b_p}, rows stacked as [b | A] (the [f | E] rows of
// the locator) with row_off[n_poly + 1].  Reference: find_extents / hit_and_run (geometry/polytope_operations.py), one numpy chain.
//
// Mapping: one LANE per chain, the 64 lanes of a wavefront are 64 chains of the SAME polytope, so the row index is wave-uniform and
// every row is fetched with scalar loads and applied to 64 chains at once.  Four wavefronts per workgroup.  The chain
// and its random stream are specified exactly in DESIGN §3.11; a numpy replay of it is tests/hit_and_run_reference.py.
//   theta, d: VGPRs for NT <= 32; for NT = 64 theta lives in LDS ([t][256 lanes], dynamic) and d in VGPRs -- 128 doubles of state
//   per lane do not fit the 256 architectural VGPRs.
// Every loop is bounded by validated inputs: n <= 64, <= 256 rows per polytope, samples * n_steps < 2^32 (mpc_hit_and_run).

// Philox4x32-10 with the Random123 constants; c is the counter on entry and the output on return
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t c1 = c[1], c3 = c[3];
        c[0] = hi1 ^ c1 ^ k0; c[1] = lo1; c[2] = hi0 ^ c3 ^ k1; c[3] = lo0;
    }
}

// a uniform double in [0, 1) from 53 bits of two words
__device__ __forceinline__ double hr_u53(uint32_t a, uint32_t b) { return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * 0x1p-53; }

constexpr int HR_BLOCK = 256;
template <int NT, bool THETA_LDS>
__global__ void __launch_bounds__(HR_BLOCK) k_hit_and_run(int n, long long n_poly, long long chains, long long waves_per_poly,
                                                          const long long *__restrict__ row_off, const double *__restrict__ ab,
                                                          const double *__restrict__ start, uint32_t samples, uint32_t n_steps,
                                                          uint32_t key0, uint32_t key1, double *__restrict__ out, int32_t *__restrict__ status) {
    extern __shared__ double hr_theta_lds[];   // THETA_LDS: [NT][HR_BLOCK]
    // the wave index is made wave-uniform explicitly, so that everything derived from it (polytope, rows) lives in SGPRs
    const long long wave = (long long)blockIdx.x * (HR_BLOCK / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= n_poly * waves_per_poly) return;
    const long long p = wave / waves_per_poly;
    const long long k = (wave - p * waves_per_poly) * 64 + (threadIdx.x & 63);
    const long long g = p * chains + k;
    const int nr = n + 1, npairs = (n + 1) / 2;
    const long long r0 = row_off[p];
    const int m = (int)(row_off[p + 1] - r0);
    const double *__restrict__ rows = ab + r0 * nr;
    double th_reg[THETA_LDS ? 1 : NT], d[NT];
    auto TH = [&](int t) -> double & {
        if constexpr (THETA_LDS) return hr_theta_lds[t * HR_BLOCK + threadIdx.x];
        else return th_reg[t];
    };
    int st = k < chains ? 0 : -1;   // -1: a lane past the last chain
#pragma unroll
    for (int t = 0; t < NT; ++t) if (t < n) TH(t) = st == 0 ? start[p * n + t] : 0.0;
    const uint32_t g_lo = (uint32_t)g, g_hi = (uint32_t)((unsigned long long)g >> 32);
    const uint32_t total = samples * n_steps;
    uint32_t until_sample = n_steps, q = 0;
    for (uint32_t s = 0; s < total; ++s) {
        if (!__any(st == 0)) break;
        if (st == 0) {
            // direction: Box-Muller pairs from calls j = 0 .. npairs-1, normalised
#pragma unroll
            for (int jp = 0; jp < (NT + 1) / 2; ++jp) {
                if (jp < npairs) {
                    uint32_t c[4] = {g_lo, g_hi, s, (uint32_t)jp};
                    philox4x32_10(c, key0, key1);
                    const double u1 = 1.0 - hr_u53(c[0], c[1]), u2 = hr_u53(c[2], c[3]);
                    const double rad = sqrt(-2.0 * log(u1));
                    double sn, cs;
                    sincospi(2.0 * u2, &sn, &cs);
                    d[2 * jp] = rad * cs;
                    if (2 * jp + 1 < NT) d[2 * jp + 1] = 2 * jp + 1 < n ? rad * sn : 0.0;
                }
            }
            double nn = 0.0;
#pragma unroll
            for (int t = 0; t < NT; ++t) if (t < n) nn += d[t] * d[t];
            const double nrm = sqrt(nn);
#pragma unroll
            for (int t = 0; t < NT; ++t) if (t < n) d[t] = d[t] / nrm;
            // one pass over the rows: slack s_i = b_i - a_i theta and rate g_i = a_i d give the chord [t_lo, t_hi]
            double t_hi = INFINITY, t_lo = -INFINITY, smin = INFINITY;
            for (int i = 0; i < m; ++i) {
                const double *a = rows + (long long)i * nr;
                double sv = a[0], gv = 0.0;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t < n) { sv = fma(-a[1 + t], TH(t), sv); gv = fma(a[1 + t], d[t], gv); }
                smin = fmin(smin, sv);
                const double ratio = sv / gv;
                if (gv > 0.0) t_hi = fmin(t_hi, ratio);
                else if (gv < 0.0) t_lo = fmax(t_lo, ratio);
            }
            if (s == 0 && smin < 0.0) st = MPC_HR_OUTSIDE;
            else if (t_hi == INFINITY || t_lo == -INFINITY) st = MPC_HR_UNBOUNDED;
            else {
                uint32_t c[4] = {g_lo, g_hi, s, (uint32_t)npairs};
                philox4x32_10(c, key0, key1);
                const double t_step = t_lo + hr_u53(c[0], c[1]) * (t_hi - t_lo);
                // acceptance: min_i (s_i - t g_i) >= 0, from the same s_i, g_i (recomputed bit for bit: same operations, same order)
                double worst = INFINITY;
                for (int i = 0; i < m; ++i) {
                    const double *a = rows + (long long)i * nr;
                    double sv = a[0], gv = 0.0;
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        if (t < n) { sv = fma(-a[1 + t], TH(t), sv); gv = fma(a[1 + t], d[t], gv); }
                    worst = fmin(worst, sv - t_step * gv);
                }
                if (worst >= 0.0) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) if (t < n) TH(t) = TH(t) + t_step * d[t];
                }
            }
        }
        if (--until_sample == 0) {
            until_sample = n_steps;
            if (st == 0) {
                double *o = out + ((size_t)g * samples + q) * n;
#pragma unroll
                for (int t = 0; t < NT; ++t) if (t < n) o[t] = TH(t);
            }
            ++q;
        }
    }
    if (st < 0) return;
    if (st > 0) {
        double *o = out + (size_t)g * samples * n;
        for (long long i = 0; i < (long long)samples * n; ++i) o[i] = __longlong_as_double(0x7ff8000000000000ll);
    }
    status[g] = st;
}


// ------------------------------------------------------------------------------------------------------------------
// k_slice_polygons: the slice of every region {theta : E theta <= f} by the plane theta = theta_c + U z (z in R^2), clipped to the box
// |z_0| <= hx, |z_1| <= hy, as a convex polygon.  z is measured from the centre of the user's box (the host shifts theta_0 to
// theta_c = theta_0 + U c), so that a small polygon far from the origin keeps its digits.  Rows are the stacked [f | E] rows of the
// locator with row_off[n_regions + 1]; plane[t] = (theta_c[t], U[t][0], U[t][1]).
//
// Mapping: one WAVEFRONT per region, four per workgroup, so the region and the row loop bounds are wave-uniform.  Lane l
// owns rows l, l + 64, ... of the region's m rows followed by the four box rows (m + 4 <= 260, so <= 5 per lane):
//   1. reduce: a_i = E_i U, beta_i = f_i - E_i theta_c, normalised to |a_i| = 1 and staged in LDS.  |a_i| <= eps |E_i| |U| is a row
//      constant on the plane: dropped if beta_i >= -eps (|f_i| + |E_i theta_c|), else the slice is empty.
//   2. clip: the line a_i z = beta_i, z = beta_i a_i + t d_i with d_i = a_i turned +90 degrees (counter-clockwise walk for an outward
//      normal), against every other row as a parametric interval [t_lo, t_hi].  A row parallel to row i (|a_j d_i| <= eps) empties
//      the line if it is tighter by more than eps D (D the box diameter), and a same-direction one within eps D of it is a
//      duplicate: the lower index keeps the edge.  Row i is an edge iff t_hi - t_lo > eps D.
//   3. rank the edges by the angle of their outward normal (counts over LDS); edge k contributes its start point as vertex k.  The
//      list is rotated to start at the vertex of smallest atan2 about the vertex mean; the area is the shoelace sum of every edge's
//      own start and end about that mean (wave reductions, butterflies: every lane holds the same bits).
// Every loop is bounded by validated inputs: n <= 64, <= 256 rows per region (mpc_slice_polygons).  No scratch (arrays of 5,
// fully unrolled).
constexpr int SP_BLOCK = 256, SP_WAVES = SP_BLOCK / 64, SP_MAX_ROWS = 256 + 4, SP_PER_LANE = (SP_MAX_ROWS + 63) / 64;

__device__ __forceinline__ double sp_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int sp_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ void __launch_bounds__(SP_BLOCK) k_slice_polygons(int n, long long n_regions, const long long *__restrict__ row_off,
                                                             const double *__restrict__ ef, const double *__restrict__ plane, double hx,
                                                             double hy, double cx, double cy, double eps, double *__restrict__ vert,
                                                             int32_t *__restrict__ edge_row, int32_t *__restrict__ count,
                                                             double *__restrict__ area, int32_t *__restrict__ status) {
    __shared__ double s_ax[SP_WAVES][SP_MAX_ROWS], s_ay[SP_WAVES][SP_MAX_ROWS], s_b[SP_WAVES][SP_MAX_ROWS], s_key[SP_WAVES][SP_MAX_ROWS];
    __shared__ int s_flag[SP_WAVES][SP_MAX_ROWS];   // 1: active row (phase 1), then 1: edge (phase 2)
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * SP_WAVES + w;
    const bool live = r < n_regions;   // wave-uniform; every wave reaches the barriers
    const long long r0 = live ? row_off[r] : 0;
    const int m = live ? (int)(row_off[r + 1] - r0) : 0, mt = live ? m + 4 : 0;
    const double D = 2.0 * sqrt(hx * hx + hy * hy), lt = eps * D;
    double unorm = 0.0;
    {
        double u0 = 0.0, u1 = 0.0;
        for (int t = 0; t < n; ++t) { u0 += plane[3 * t + 1] * plane[3 * t + 1]; u1 += plane[3 * t + 2] * plane[3 * t + 2]; }
        unorm = sqrt(fmax(u0, u1));
    }
    // 1. reduce every row to the plane
    int violated = 0;
#pragma unroll
    for (int k = 0; k < SP_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        if (i >= mt) continue;
        double ax, ay, b;
        int act = 1;
        if (i < m) {
            const double *row = ef + (r0 + i) * (long long)(n + 1);
            const double f = row[0];
            double dot = 0.0, ee = 0.0;
            ax = 0.0; ay = 0.0;
            for (int t = 0; t < n; ++t) {
                const double e = row[1 + t];
                ax += e * plane[3 * t + 1];
                ay += e * plane[3 * t + 2];
                dot += e * plane[3 * t];
                ee += e * e;
            }
            b = f - dot;
            const double nrm = sqrt(ax * ax + ay * ay);
            if (nrm <= eps * sqrt(ee) * unorm) {
                act = 0;
                if (b < -eps * (fabs(f) + fabs(dot))) violated = 1;
            } else {
                ax /= nrm; ay /= nrm; b /= nrm;
            }
        } else {   // box rows -1 .. -4: z_0 <= hx, z_1 <= hy, -z_0 <= hx, -z_1 <= hy
            const int s = i - m;
            ax = s == 0 ? 1.0 : s == 2 ? -1.0 : 0.0;
            ay = s == 1 ? 1.0 : s == 3 ? -1.0 : 0.0;
            b = (s & 1) ? hy : hx;
        }
        s_ax[w][i] = ax; s_ay[w][i] = ay; s_b[w][i] = b; s_flag[w][i] = act;
    }
    __syncthreads();
    // 2. clip the line of every active row against all others
    double sx[SP_PER_LANE], sy[SP_PER_LANE], ex[SP_PER_LANE], ey[SP_PER_LANE];
    int edge[SP_PER_LANE];
    int nonempty = 0;
#pragma unroll
    for (int k = 0; k < SP_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        edge[k] = 0; sx[k] = sy[k] = ex[k] = ey[k] = 0.0;
        if (i >= mt || !s_flag[w][i]) continue;
        const double ax = s_ax[w][i], ay = s_ay[w][i], bi = s_b[w][i];
        const double px = bi * ax, py = bi * ay, dx = -ay, dy = ax;
        double tlo = -INFINITY, thi = INFINITY;
        bool dead = false;
        for (int j = 0; j < mt; ++j) {
            if (j == i || !s_flag[w][j]) continue;
            const double bx = s_ax[w][j], by = s_ay[w][j];
            const double den = bx * dx + by * dy;
            const double num = s_b[w][j] - (bx * px + by * py);
            if (fabs(den) <= eps) {
                if (num < -lt) dead = true;                                                 // a tighter parallel row
                else if (num <= lt && bx * ax + by * ay > 0.0 && j < i) dead = true;        // a duplicate with a lower index
            } else if (den > 0.0) thi = fmin(thi, num / den);
            else tlo = fmax(tlo, num / den);
        }
        if (!dead && thi - tlo >= -lt) nonempty = 1;
        if (!dead && thi - tlo > lt) {
            edge[k] = 1;
            sx[k] = px + tlo * dx; sy[k] = py + tlo * dy;
            ex[k] = px + thi * dx; ey[k] = py + thi * dy;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SP_PER_LANE; ++k) {
        const int i = lane + 64 * k;
        if (i >= mt) continue;
        s_flag[w][i] = edge[k];
        s_key[w][i] = atan2(s_ay[w][i], s_ax[w][i]);
    }
    __syncthreads();
    if (!live) return;   // no barrier below
    // 3. order, mean, area, start
    int mine = 0;
    double mx = 0.0, my = 0.0;
#pragma unroll
    for (int k = 0; k < SP_PER_LANE; ++k) if (edge[k]) { ++mine; mx += sx[k]; my += sy[k]; }
    const int nv = sp_wave_sum(mine);
    violated = sp_wave_sum(violated);
    nonempty = sp_wave_sum(nonempty);
    mx = sp_wave_sum(mx); my = sp_wave_sum(my);
    int st;
    if (violated || (nv == 0 && !nonempty)) st = MPC_SLICE_EMPTY;
    else {
        mx /= nv > 0 ? nv : 1; my /= nv > 0 ? nv : 1;
        int rank[SP_PER_LANE];
        double ang_min = INFINITY, a2 = 0.0;
        int rank_min = 0, cut = 0;
#pragma unroll
        for (int k = 0; k < SP_PER_LANE; ++k) {
            const int i = lane + 64 * k;
            rank[k] = 0;
            if (!edge[k]) continue;
            const double key = s_key[w][i];
            int rk = 0;
            for (int j = 0; j < mt; ++j) rk += s_flag[w][j] && (s_key[w][j] < key || (s_key[w][j] == key && j < i));
            rank[k] = rk;
            const double ang = atan2(sy[k] - my, sx[k] - mx);
            if (ang < ang_min || (ang == ang_min && rk < rank_min)) { ang_min = ang; rank_min = rk; }
            a2 += (sx[k] - mx) * (ey[k] - my) - (sy[k] - my) * (ex[k] - mx);
            if (i >= m) cut = 1;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double oa = __shfl_xor(ang_min, off);
            const int orank = __shfl_xor(rank_min, off);
            if (oa < ang_min || (oa == ang_min && orank < rank_min)) { ang_min = oa; rank_min = orank; }
        }
        const double ar = 0.5 * sp_wave_sum(a2);
        cut = sp_wave_sum(cut);
        st = (nv < 3 || ar <= eps * D * D) ? MPC_SLICE_LOWDIM : MPC_SLICE_FULL;
        if (cut) st |= MPC_SLICE_CUT;
        const long long vo = r0 + 4 * r;
#pragma unroll
        for (int k = 0; k < SP_PER_LANE; ++k) {
            const int i = lane + 64 * k;
            if (!edge[k]) continue;
            const long long q = vo + (rank[k] - rank_min + nv) % nv;
            vert[2 * q] = sx[k] + cx;
            vert[2 * q + 1] = sy[k] + cy;
            edge_row[q] = i < m ? i : -(i - m + 1);
        }
        if (lane == 0) { count[r] = nv; area[r] = ar; }
    }
    if (lane == 0) {
        status[r] = st;
        if (st == MPC_SLICE_EMPTY) { count[r] = 0; area[r] = 0.0; }
    }
}

// k_slice_intervals: the slice of every region by the line theta = theta_0 + u t, clipped to [t_lo, t_hi]; one wavefront per region,
// lanes over its rows, min / max by wave butterflies.  |E_i u| <= eps |E_i| |u| is a row constant on the line (as in k_slice_polygons).
__global__ void __launch_bounds__(SP_BLOCK) k_slice_intervals(int n, long long n_regions, const long long *__restrict__ row_off,
                                                              const double *__restrict__ ef, const double *__restrict__ line, double t_lo,
                                                              double t_hi, double eps, double *__restrict__ interval,
                                                              int32_t *__restrict__ status) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * SP_WAVES + w;
    if (r >= n_regions) return;
    const long long r0 = row_off[r];
    const int m = (int)(row_off[r + 1] - r0);
    double uu = 0.0;
    for (int t = 0; t < n; ++t) uu += line[2 * t + 1] * line[2 * t + 1];
    const double unorm = sqrt(uu);
    double lo = -INFINITY, hi = INFINITY;
    int violated = 0;
    for (int i = lane; i < m; i += 64) {
        const double *row = ef + (r0 + i) * (long long)(n + 1);
        const double f = row[0];
        double a = 0.0, dot = 0.0, ee = 0.0;
        for (int t = 0; t < n; ++t) {
            const double e = row[1 + t];
            a += e * line[2 * t + 1];
            dot += e * line[2 * t];
            ee += e * e;
        }
        const double b = f - dot;
        if (fabs(a) <= eps * sqrt(ee) * unorm) { if (b < -eps * (fabs(f) + fabs(dot))) violated = 1; }
        else if (a > 0.0) hi = fmin(hi, b / a);
        else lo = fmax(lo, b / a);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fmax(lo, __shfl_xor(lo, off));
        hi = fmin(hi, __shfl_xor(hi, off));
        violated |= __shfl_xor(violated, off);
    }
    if (lane) return;
    const double L = t_hi - t_lo, a = fmax(lo, t_lo), b = fmin(hi, t_hi);
    int st;
    if (violated || b - a < -eps * L) st = MPC_SLICE_EMPTY;
    else st = (b - a <= eps * L ? MPC_SLICE_LOWDIM : MPC_SLICE_FULL) | (lo <= t_lo || hi >= t_hi ? MPC_SLICE_CUT : 0);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    interval[2 * r] = st == MPC_SLICE_EMPTY ? nan : a;
    interval[2 * r + 1] = st == MPC_SLICE_EMPTY ? nan : fmax(a, b);
    status[r] = st;
}

}  // namespace mpc
