// closed_loop.hpp -- explicit controllers in closed loop (gfx950); DESIGN §3.15.
//
// One LANE per trajectory, all `steps` steps inside one launch; a lane's theta lives in registers.  One step of trajectory p at theta_k:
//   1. j_k = the region Solution.get_region_batch(theta_k) returns, with the scan's row test and rule (loc_row_inside / loc_objective,
//      locate.hpp), found by one of three locators:
//        SIM_SCAN        the wavefront-cooperative list scan of k_locate (loc_scan_block): every lane of a workgroup is at the same step;
//        SIM_TREE        the descent of the attached search tree (loc_tree, tree.hpp);
//        SIM_WALK2 / 4   the adjacency walk (loc_walk, locate.hpp) started at the lane's previous region (2 / 4 mask words);
//      a point the tree or the walk leaves unresolved (-2) is settled by the lane's own list scan (loc_scan_lane), counted as a fallback;
//   2. j_k = -1 ends the trajectory with status 2;
//   3. u_k = x*(theta_k)[inputs]: the fma chain of k_evaluate;
//   4. theta_{k+1,i} = c_i + A_i0 theta_0 + ... + B_i0 u_0 + ... + w_i, term by term, one rounded product and one rounded sum each (no
//      fma: the library builds with -ffp-contract=off), so that a numpy replay in the same order is bit-exact.  Without c the sum starts
//      at 0.0; without a disturbance there is no w term.
// A state with a non-finite component ends the trajectory before its step (status 3); |theta_{k+1} - theta_k|_inf <= stop_tol (stop_tol
// >= 0) ends it after the step (status 1).
// Outputs are step-major ([k][p][.]: the stores of a wavefront are contiguous); the host fills them with NaN / -1 before the launch, and
// nothing after a trajectory's end is written.  The disturbance is none, an array [k][p][t], or the box lo + (hi - lo) U with U = hr_u53
// of Philox4x32-10 under (key0, key1) at the counter (p_lo, p_hi, k, j): w_2j from words 0, 1, w_2j+1 from words 2, 3.
#pragma once
#include <stdint.h>

#include "locate.hpp"
#include "tree.hpp"

namespace mpc {

constexpr int SIM_SCAN = 0, SIM_TREE = 1, SIM_WALK2 = 2, SIM_WALK4 = 3;
constexpr int SIM_BLOCK = 256;

struct SimArgs {
    long long n;                                   // trajectories
    int steps, nt, nx, nu;
    // the locator's rows and laws
    long long n_regions, n_rows;
    const long long *row_off;
    const int32_t *row_region, *row_end;
    const double *ef, *xlaw, *Q, *cvec, *H;
    double tol;
    int overlapping, inclusive;
    // the walk
    const int32_t *row_info, *sorted_region;
    const unsigned long long *masks, *sorted_masks;
    int n_c, max_walk;
    // the tree
    const double *planes, *node_tau;
    const int32_t *node_plane, *node_child, *items;
    const long long *node_off;
    // the plant
    const double *theta0;                          // [n][nt]
    const int32_t *inputs;                         // [nu]
    const double *A, *B, *c;                       // [nt][nt], [nt][nu], [nt] (c may be NULL)
    const double *w;                               // [steps][n][nt] or NULL
    const double *lo, *hi;                         // [nt] box or NULL
    uint32_t key0, key1;
    double stop_tol;                               // < 0: off
    int final_only;
    // outputs
    double *theta;                                 // [steps + 1][n][nt], or [n][nt] with final_only
    double *u;                                     // [steps][n][nu]
    int32_t *region;                               // [steps][n]
    int32_t *status, *exit_step;                   // [n]
    unsigned long long *counters;                  // [0] trajectory steps, [1] walk crossings, [2] fallbacks
};

template <int NT, int NU, int MODE>
__global__ void __launch_bounds__(SIM_BLOCK) k_simulate(SimArgs a) {
    constexpr int TILE = MODE == SIM_SCAN ? LOC_TILE : 1, STK = MODE == SIM_TREE ? TR_STACK : 1;
    __shared__ double tile[TILE][NT + 1];
    __shared__ int trid[TILE], tend[TILE];
    __shared__ int stack[STK * SIM_BLOCK];
    const long long n = a.n, p = (long long)blockIdx.x * SIM_BLOCK + threadIdx.x;
    const int nt = a.nt, nu = a.nu, nr = nt + 1;
    const bool live = p < n;
    double th[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) th[t] = live && t < nt ? a.theta0[p * nt + t] : 0.0;
    if (live && !a.final_only) {
#pragma unroll
        for (int t = 0; t < NT; ++t) if (t < nt) a.theta[p * nt + t] = th[t];
    }
    int st = live ? -1 : 0, ex = a.steps;          // st -1: running
    long long prev = 0;                            // the walk's start: the previous region
    unsigned long long n_steps = 0, n_cross = 0, n_fb = 0;
    const uint32_t p_lo = (uint32_t)p, p_hi = (uint32_t)((unsigned long long)p >> 32);
    for (int k = 0; k < a.steps; ++k) {
        if constexpr (MODE == SIM_SCAN) {
            if (!__syncthreads_or(st == -1)) break;   // the scan stages rows with barriers: the whole workgroup goes on together
        } else {
            if (st != -1) break;
        }
        bool run = st == -1;
        if (run) {
            bool fin = true;
#pragma unroll
            for (int t = 0; t < NT; ++t) if (t < nt) fin = fin && isfinite(th[t]);
            if (!fin) { st = 3; ex = k; run = false; }
        }
        long long r = -1;
        if constexpr (MODE == SIM_SCAN) {
            r = loc_scan_block<NT>(run, th, nt, a.nx, a.n_rows, a.row_region, a.row_end, a.ef, a.xlaw, a.Q, a.cvec, a.H, a.tol, a.overlapping,
                                   a.inclusive, tile, trid, tend);
        } else if (run) {
            if constexpr (MODE == SIM_TREE)
                r = loc_tree<NT>(th, nt, a.nx, a.planes, a.node_plane, a.node_child, a.node_tau, a.node_off, a.items, a.row_off, a.ef, a.xlaw, a.Q,
                                 a.cvec, a.H, a.tol, a.overlapping, a.inclusive, stack);
            else
                r = loc_walk<NT, MODE == SIM_WALK2 ? 2 : 4>(th, nt, a.n_regions, a.row_off, a.ef, a.row_info, a.masks, a.sorted_masks,
                                                            a.sorted_region, a.tol, prev, a.max_walk, a.n_c, n_cross);
            if (r == -2) {
                r = loc_scan_lane<NT>(th, nt, a.nx, a.n_regions, a.row_off, a.ef, a.xlaw, a.Q, a.cvec, a.H, a.tol, a.overlapping, a.inclusive);
                ++n_fb;
            }
        }
        if (!run) continue;
        ++n_steps;
        if (r < 0) { st = 2; ex = k; continue; }
        prev = r;
        // u_k: the rows `inputs` of the law, formed as k_evaluate forms them
        double uu[NU];
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            uu[i] = 0.0;
            if (i < nu) {
                const double *row = a.xlaw + ((size_t)r * a.nx + a.inputs[i]) * nr;
                double v = row[0];
#pragma unroll
                for (int t = 0; t < NT; ++t) if (t < nt) v = fma(row[1 + t], th[t], v);
                uu[i] = v;
            }
        }
        // theta_{k+1}: c, then the A terms, the B terms and w, in this order, without fma
        double tn[NT];
        uint32_t rnd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            tn[i] = 0.0;
            if (i < nt) {
                double v = a.c ? a.c[i] : 0.0;
#pragma unroll
                for (int j = 0; j < NT; ++j) if (j < nt) v = v + a.A[i * nt + j] * th[j];
#pragma unroll
                for (int l = 0; l < NU; ++l) if (l < nu) v = v + a.B[i * nu + l] * uu[l];
                if (a.w) {
                    v = v + a.w[((size_t)k * n + p) * nt + i];
                } else if (a.lo) {
                    if ((i & 1) == 0) {
                        rnd[0] = p_lo; rnd[1] = p_hi; rnd[2] = (uint32_t)k; rnd[3] = (uint32_t)(i >> 1);
                        philox4x32_10(rnd, a.key0, a.key1);
                    }
                    const double U = (i & 1) ? hr_u53(rnd[2], rnd[3]) : hr_u53(rnd[0], rnd[1]);
                    v = v + (a.lo[i] + (a.hi[i] - a.lo[i]) * U);
                }
                tn[i] = v;
            }
        }
        if (!a.final_only) {
            a.region[(size_t)k * n + p] = (int32_t)r;
#pragma unroll
            for (int i = 0; i < NU; ++i) if (i < nu) a.u[((size_t)k * n + p) * nu + i] = uu[i];
#pragma unroll
            for (int t = 0; t < NT; ++t) if (t < nt) a.theta[((size_t)(k + 1) * n + p) * nt + t] = tn[t];
        }
        bool steady = a.stop_tol >= 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) if (t < nt) { steady = steady && fabs(tn[t] - th[t]) <= a.stop_tol; th[t] = tn[t]; }
        if (steady) { st = 1; ex = k + 1; }
    }
    if (st == -1) st = 0;
    if (live) {
        if (a.final_only) {
#pragma unroll
            for (int t = 0; t < NT; ++t) if (t < nt) a.theta[p * nt + t] = th[t];
        }
        a.status[p] = st;
        a.exit_step[p] = ex;
    }
    // counters: wave sums, one atomic each per wavefront (every lane reaches this point)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_steps += __shfl_xor(n_steps, off);
        n_cross += __shfl_xor(n_cross, off);
        n_fb += __shfl_xor(n_fb, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(a.counters + 0, n_steps);
        atomicAdd(a.counters + 1, n_cross);
        atomicAdd(a.counters + 2, n_fb);
    }
}

}  // namespace mpc
