// geometry.hip -- the stateless geometry entry points of the C ABI (include/mpcombi.h): hit-and-run sampling, slices, point
// location (list scan, adjacency walk, search tree), tree build, closed-loop simulation, vertex enumeration, region volumes and region
// merging and the overlap removal.  None of them knows mpc_handle; each is a batch in, one or a few launches, the results out.  Their kernels are compiled here
// and nowhere else (locate.hpp, tree.hpp, closed_loop.hpp, vertices.hpp, volume.hpp, merge.hpp, overlap.hpp, transition.hpp, exit_sets.hpp, reduce.hpp, project.hpp, simplex.hpp); the pools and the scaffold
// of a one-shot call (OneShot, select_device) are host_common.hpp.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mpcombi.h"
#include "locate.hpp"
#include "tree.hpp"
#include "closed_loop.hpp"
#include "vertices.hpp"
#include "volume.hpp"
#include "merge.hpp"
#include "overlap.hpp"
#include "transition.hpp"
#include "exit_sets.hpp"
#include "reduce.hpp"
#include "support.hpp"
#include "project.hpp"
#include "invariant.hpp"
#include "forward.hpp"
#include "compare.hpp"
#include "box_pairs.hpp"
#include "host_common.hpp"

using namespace mpc;

// the refusal of an entry point: MPC_ERR_INVALID with the message "<who>: <why>"
static int bad(const char *who, const std::string &why) { return fail(nullptr, MPC_ERR_INVALID, std::string(who) + ": " + why); }

// the two arrays every batch of polytopes starts with: row_off [n + 1] and the rows [row_off[n]][width]
struct RegionsOnDevice { DevBuf &off, &ef; };
static RegionsOnDevice upload_regions(OneShot &s, int64_t n, const int64_t *row_off, const double *rows, int width) {
    DevBuf &off = s.upload(row_off, (size_t)(n + 1) * 8);
    return {off, s.upload(rows, (size_t)row_off[n] * width * 8)};
}

// f(std::integral_constant<int, W>) with the kernels' compile-time width of nt parameters: W = 4, 8 or 16
template <class F> static decltype(auto) with_width(int nt, F &&f) {
    if (nt <= 4) return f(std::integral_constant<int, 4>{});
    if (nt <= 8) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, 16>{});
}

// ---- hit-and-run chains in a batch of polytopes (k_hit_and_run, locate.hpp) -----------------------------------------------
template <int NT, bool L>
static void hr_launch(dim3 g, size_t lds, int n, long long n_poly, long long chains, long long wpp, const DevBuf &off, const DevBuf &ab,
                      const DevBuf &st0, uint32_t samples, uint32_t n_steps, uint32_t k0, uint32_t k1, DevBuf &out, DevBuf &status) {
    hipLaunchKernelGGL((k_hit_and_run<NT, L>), g, dim3(HR_BLOCK), lds, nullptr, n, n_poly, chains, wpp, off.as<long long>(), ab.as<double>(),
                       st0.as<double>(), samples, n_steps, k0, k1, out.as<double>(), status.as<int32_t>());
}

extern "C" int mpc_hit_and_run(int32_t device, int32_t n, int64_t n_poly, const int64_t *row_off, const double *ab_rows, const double *start,
                               int64_t chains, int64_t samples, int64_t n_steps, uint64_t seed, double *out, int32_t *status, float *ms) {
    if (ms) *ms = 0.0f;
    if (n < 1 || n > 64) return fail(nullptr, MPC_ERR_INVALID, "mpc_hit_and_run: n must lie in 1..64");
    if (n_poly < 0 || chains < 0 || samples < 1 || n_steps < 1) return fail(nullptr, MPC_ERR_INVALID, "mpc_hit_and_run: bad sizes");
    if (samples >= (1ll << 32) || n_steps >= (1ll << 32) || (unsigned long long)samples * (unsigned long long)n_steps >= (1ull << 32))
        return fail(nullptr, MPC_ERR_INVALID, "mpc_hit_and_run: samples * n_steps must stay below 2^32");
    if (!row_off) return fail(nullptr, MPC_ERR_INVALID, "mpc_hit_and_run: missing row_off");
    if (row_off[0] != 0) return fail(nullptr, MPC_ERR_INVALID, "mpc_hit_and_run: row_off[0] must be 0");
    for (int64_t p = 0; p < n_poly; ++p) {
        const int64_t r = row_off[p + 1] - row_off[p];
        if (r < 0 || r > 256) return fail(nullptr, MPC_ERR_INVALID, "mpc_hit_and_run: a polytope has more than 256 rows (or row_off decreases)");
    }
    if (n_poly == 0 || chains == 0) return MPC_OK;
    if ((row_off[n_poly] && !ab_rows) || !start || !out || !status) return fail(nullptr, MPC_ERR_INVALID, "mpc_hit_and_run: missing array");
    const long long wpp = (chains + 63) / 64;
    if (n_poly > (1ll << 40) / wpp) return fail(nullptr, MPC_ERR_INVALID, "mpc_hit_and_run: too many chains");
    const long long n_blocks = (n_poly * wpp + HR_BLOCK / 64 - 1) / (HR_BLOCK / 64);
    if (n_blocks > 0x7fffffffll) return fail(nullptr, MPC_ERR_INVALID, "mpc_hit_and_run: too many chains for one launch");
    if (int rc = select_device(nullptr, device)) return rc;
    const size_t n_chain = (size_t)n_poly * chains, n_out = n_chain * samples * n;
    const int nt = n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64;
    const size_t lds = nt == 64 ? (size_t)64 * HR_BLOCK * sizeof(double) : 0;
    if (lds > 48 * 1024) HIP_TRY(nullptr, hipFuncSetAttribute(reinterpret_cast<const void *>(k_hit_and_run<64, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    OneShot s("mpc_hit_and_run", nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_poly, row_off, ab_rows, n + 1);
    DevBuf &d_st0 = s.upload(start, (size_t)n_poly * n * 8), &d_out = s.buf(n_out * 8), &d_status = s.buf(n_chain * 4);
    s.launch_timed([&] {
        const dim3 g((unsigned)n_blocks);
        const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), sm = (uint32_t)samples, ns = (uint32_t)n_steps;
        switch (nt) {
            case 2: hr_launch<2, false>(g, 0, n, n_poly, chains, wpp, d.off, d.ef, d_st0, sm, ns, k0, k1, d_out, d_status); break;
            case 4: hr_launch<4, false>(g, 0, n, n_poly, chains, wpp, d.off, d.ef, d_st0, sm, ns, k0, k1, d_out, d_status); break;
            case 8: hr_launch<8, false>(g, 0, n, n_poly, chains, wpp, d.off, d.ef, d_st0, sm, ns, k0, k1, d_out, d_status); break;
            case 16: hr_launch<16, false>(g, 0, n, n_poly, chains, wpp, d.off, d.ef, d_st0, sm, ns, k0, k1, d_out, d_status); break;
            case 32: hr_launch<32, false>(g, 0, n, n_poly, chains, wpp, d.off, d.ef, d_st0, sm, ns, k0, k1, d_out, d_status); break;
            default: hr_launch<64, true>(g, lds, n, n_poly, chains, wpp, d.off, d.ef, d_st0, sm, ns, k0, k1, d_out, d_status); break;
        }
    });
    s.download(out, d_out, n_out * 8);
    s.download(status, d_status, n_chain * 4);
    s.elapsed(ms);
    return s.finish();
}

// ---- slices of a batch of polytopes by a plane or a line (k_slice_polygons / k_slice_intervals, locate.hpp) ---------------------
static int slice_check(const char *who, int32_t n, int64_t n_regions, const int64_t *row_off, double eps) {
    char msg[160];
    if (n < 1 || n > 64) { snprintf(msg, sizeof msg, "%s: n must lie in 1..64", who); return fail(nullptr, MPC_ERR_INVALID, msg); }
    if (n_regions < 0 || !row_off || row_off[0] != 0) { snprintf(msg, sizeof msg, "%s: bad n_regions or row_off", who); return fail(nullptr, MPC_ERR_INVALID, msg); }
    if (!(eps > 0.0 && eps < 1.0)) { snprintf(msg, sizeof msg, "%s: eps must lie in (0, 1)", who); return fail(nullptr, MPC_ERR_INVALID, msg); }
    for (int64_t r = 0; r < n_regions; ++r) {
        const int64_t k = row_off[r + 1] - row_off[r];
        if (k < 0 || k > 256) { snprintf(msg, sizeof msg, "%s: a region has more than 256 rows (or row_off decreases)", who); return fail(nullptr, MPC_ERR_INVALID, msg); }
    }
    if (n_regions > 4ll * 0x7fffffffll) { snprintf(msg, sizeof msg, "%s: too many regions for one launch", who); return fail(nullptr, MPC_ERR_INVALID, msg); }
    return MPC_OK;
}

// one launch of a slice kernel with its inputs copied in and its outputs copied out; launch(d_in...) enqueues the kernel
template <class Launch>
static int slice_run(const char *who, int32_t device, int64_t n_regions, const int64_t *row_off, const double *ef_rows, int32_t n,
                     const std::vector<double> &param, std::initializer_list<std::pair<void *, size_t>> outs, float *ms, Launch launch) {
    if (int rc = select_device(nullptr, device)) return rc;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_regions, row_off, ef_rows, n + 1);
    DevBuf &d_param = s.upload(param.data(), param.size() * 8);
    DevBuf *d_out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    { size_t q = 0; for (auto &o : outs) d_out[q++] = &s.buf(std::max<size_t>(8, o.second)); }
    s.launch_timed([&] { launch(dim3((unsigned)((n_regions + SP_WAVES - 1) / SP_WAVES)), d.off.as<long long>(), d.ef.as<double>(), d_param.as<double>(), d_out); });
    { size_t q = 0; for (auto &o : outs) s.download(o.first, *d_out[q++], o.second); }
    s.elapsed(ms);
    return s.finish();
}

extern "C" int mpc_slice_polygons(int32_t device, int32_t n, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *theta0,
                                  const double *U, const double *box, double eps, double *vert, int32_t *edge_row, int32_t *count, double *area,
                                  int32_t *status, float *ms) {
    if (ms) *ms = 0.0f;
    if (int rc = slice_check("mpc_slice_polygons", n, n_regions, row_off, eps)) return rc;
    if (!theta0 || !U || !box) return fail(nullptr, MPC_ERR_INVALID, "mpc_slice_polygons: missing theta0, U or box");
    for (int k = 0; k < 2; ++k)
        if (!std::isfinite(box[k]) || !std::isfinite(box[k + 2]) || !(box[k] < box[k + 2]))
            return fail(nullptr, MPC_ERR_INVALID, "mpc_slice_polygons: the box must be finite with lo < hi");
    if (n_regions == 0) return MPC_OK;
    const long long rows = row_off[n_regions], slots = rows + 4 * n_regions;
    if ((rows && !ef_rows) || !vert || !edge_row || !count || !area || !status) return fail(nullptr, MPC_ERR_INVALID, "mpc_slice_polygons: missing array");
    // z is measured from the box centre c: plane[t] = (theta0 + U c, U[t][0], U[t][1])
    const double cx = 0.5 * (box[0] + box[2]), cy = 0.5 * (box[1] + box[3]), hx = 0.5 * (box[2] - box[0]), hy = 0.5 * (box[3] - box[1]);
    std::vector<double> plane(3 * (size_t)n);
    for (int t = 0; t < n; ++t) {
        plane[3 * t] = theta0[t] + U[2 * t] * cx + U[2 * t + 1] * cy;
        plane[3 * t + 1] = U[2 * t];
        plane[3 * t + 2] = U[2 * t + 1];
    }
    return slice_run("mpc_slice_polygons", device, n_regions, row_off, ef_rows, n, plane,
                     {{vert, (size_t)slots * 16}, {edge_row, (size_t)slots * 4}, {count, (size_t)n_regions * 4}, {area, (size_t)n_regions * 8},
                      {status, (size_t)n_regions * 4}}, ms,
                     [&](dim3 g, const long long *off, const double *ef, const double *prm, DevBuf *const *o) {
                         hipLaunchKernelGGL(k_slice_polygons, g, dim3(SP_BLOCK), 0, nullptr, n, (long long)n_regions, off, ef, prm, hx, hy, cx, cy, eps,
                                            o[0]->as<double>(), o[1]->as<int32_t>(), o[2]->as<int32_t>(), o[3]->as<double>(), o[4]->as<int32_t>());
                     });
}

extern "C" int mpc_slice_intervals(int32_t device, int32_t n, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *theta0,
                                   const double *u, double t_lo, double t_hi, double eps, double *interval, int32_t *status, float *ms) {
    if (ms) *ms = 0.0f;
    if (int rc = slice_check("mpc_slice_intervals", n, n_regions, row_off, eps)) return rc;
    if (!theta0 || !u) return fail(nullptr, MPC_ERR_INVALID, "mpc_slice_intervals: missing theta0 or u");
    if (!std::isfinite(t_lo) || !std::isfinite(t_hi) || !(t_lo < t_hi)) return fail(nullptr, MPC_ERR_INVALID, "mpc_slice_intervals: the range must be finite with t_lo < t_hi");
    if (n_regions == 0) return MPC_OK;
    if ((row_off[n_regions] && !ef_rows) || !interval || !status) return fail(nullptr, MPC_ERR_INVALID, "mpc_slice_intervals: missing array");
    std::vector<double> line(2 * (size_t)n);
    for (int t = 0; t < n; ++t) { line[2 * t] = theta0[t]; line[2 * t + 1] = u[t]; }
    return slice_run("mpc_slice_intervals", device, n_regions, row_off, ef_rows, n, line,
                     {{interval, (size_t)n_regions * 16}, {status, (size_t)n_regions * 4}}, ms,
                     [&](dim3 g, const long long *off, const double *ef, const double *prm, DevBuf *const *o) {
                         hipLaunchKernelGGL(k_slice_intervals, g, dim3(SP_BLOCK), 0, nullptr, n, (long long)n_regions, off, ef, prm, t_lo, t_hi, eps,
                                            o[0]->as<double>(), o[1]->as<int32_t>());
                     });
}

struct mpc_locator {
    int device = 0, n_x = 0, n_t = 0;
    long long n_regions = 0, n_rows = 0;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    DevBuf row_off, row_region, row_end, ef, xlaw, Q, c, H, theta, region, x;
    // adjacency for the walk (mpc_locator_set_adjacency): active-set masks in region order and sorted, facet kind / id per row
    DevBuf masks, sorted_masks, sorted_region, row_info, theta2, region2;
    int mask_words = 0, n_c = 0;
    bool has_adj = false;
    long long last_unresolved = 0;   // points of the last walk query that went to the list scan
    bool hasQ = false, hasc = false, hasH = false;
    std::vector<int64_t> h_row_off;  // host copy of row_off (limits of mpc_tree_build)
    // search tree (mpc_tree_build / mpc_locator_set_tree): host arrays as attached, and their device copies
    bool has_tree = false;
    double tree_tol = 0.0;
    int tree_planes = 0;
    std::vector<double> h_planes, h_tau;
    std::vector<int32_t> h_plane, h_child, h_items;
    std::vector<int64_t> h_off;
    DevBuf t_planes, t_plane, t_child, t_tau, t_off, t_items;
};

static int locator_fill(mpc_locator *L, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *xlaw, const double *Q,
                        const double *c, const double *H);
extern "C" int mpc_locator_destroy(mpc_locator *L);

// host -> device on the locator's stream into b, grown to max(8, bytes); nothing is copied when bytes == 0
static hipError_t locator_upload(mpc_locator *L, DevBuf &b, const void *src, size_t bytes) {
    hipError_t e = b.ensure(std::max<size_t>(bytes, 8), L->stream);
    if (e != hipSuccess || !bytes) return e;
    return hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, L->stream);
}

extern "C" int mpc_locator_create(int32_t device, int32_t n_x, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows,
                                  const double *xlaw, const double *Q, const double *c, const double *H, mpc_locator **out) {
    if (!out || n_x < 1 || n_t < 1 || n_t > 16 || n_regions < 0 || (n_regions > 0 && (!row_off || !ef_rows || !xlaw)))
        return fail(nullptr, MPC_ERR_INVALID, "mpc_locator_create: bad arguments (1 <= n_t <= 16)");
    HIP_TRY(nullptr, hipSetDevice(device));
    mpc_locator *L = new mpc_locator();
    L->device = device; L->n_x = n_x; L->n_t = n_t; L->n_regions = n_regions;
    const int rc_fill = locator_fill(L, n_regions, row_off, ef_rows, xlaw, Q, c, H);
    if (rc_fill != MPC_OK) { (void)mpc_locator_destroy(L); return rc_fill; }   // one cleanup path: nothing leaks on failure
    *out = L;
    return MPC_OK;
}

static int locator_fill(mpc_locator *L, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *xlaw, const double *Q,
                        const double *c, const double *H) {
    const int n_x = L->n_x, n_t = L->n_t;
    HIP_TRY(nullptr, hipStreamCreateWithFlags(&L->stream, hipStreamNonBlocking));
    HIP_TRY(nullptr, hipEventCreate(&L->e0));
    HIP_TRY(nullptr, hipEventCreate(&L->e1));
    const long long rows = n_regions ? row_off[n_regions] : 0;
    L->n_rows = rows;
    L->h_row_off.assign(row_off, row_off + (n_regions ? n_regions + 1 : 0));
    if (!n_regions) L->h_row_off.assign(1, 0);
    const long long zero = 0;
    HIP_TRY(nullptr, locator_upload(L, L->row_off, n_regions ? (const void *)row_off : (const void *)&zero, (size_t)(n_regions + 1) * sizeof(int64_t)));
    HIP_TRY(nullptr, locator_upload(L, L->ef, ef_rows, (size_t)rows * (n_t + 1) * sizeof(double)));
    std::vector<int32_t> rr((size_t)std::max<long long>(rows, 1)), re((size_t)std::max<long long>(rows, 1));
    for (long long r = 0; r < n_regions; ++r)
        for (long long i = row_off[r]; i < row_off[r + 1]; ++i) { rr[(size_t)i] = (int32_t)r; re[(size_t)i] = (int32_t)row_off[r + 1]; }
    HIP_TRY(nullptr, locator_upload(L, L->row_region, rr.data(), (size_t)rows * sizeof(int32_t)));
    HIP_TRY(nullptr, locator_upload(L, L->row_end, re.data(), (size_t)rows * sizeof(int32_t)));
    HIP_TRY(nullptr, locator_upload(L, L->xlaw, xlaw, (size_t)n_regions * n_x * (n_t + 1) * sizeof(double)));
    if (Q) { HIP_TRY(nullptr, locator_upload(L, L->Q, Q, (size_t)n_x * n_x * sizeof(double))); L->hasQ = true; }
    if (c) { HIP_TRY(nullptr, locator_upload(L, L->c, c, (size_t)n_x * sizeof(double))); L->hasc = true; }
    if (H) { HIP_TRY(nullptr, locator_upload(L, L->H, H, (size_t)n_x * n_t * sizeof(double))); L->hasH = true; }
    HIP_TRY(nullptr, hipStreamSynchronize(L->stream));
    return MPC_OK;
}

extern "C" int mpc_locator_set_adjacency(mpc_locator *L, int32_t mask_words, int32_t n_c, const uint64_t *masks, const int32_t *row_info) {
    if (!L || !masks || !row_info || (mask_words != 2 && mask_words != 4) || n_c < 1 || n_c > 64 * mask_words) return MPC_ERR_INVALID;
    HIP_TRY(nullptr, hipSetDevice(L->device));
    const long long n = L->n_regions, rows = L->n_rows;
    if (n <= 0) return MPC_OK;
    const int mw = mask_words;
    // the mask table sorted ascending (most significant word last), with the region each mask belongs to
    std::vector<int32_t> order((size_t)n);
    for (long long i = 0; i < n; ++i) order[(size_t)i] = (int32_t)i;
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        for (int j = mw - 1; j >= 0; --j) { const uint64_t va = masks[(size_t)a * mw + j], vb = masks[(size_t)b * mw + j]; if (va != vb) return va < vb; }
        return a < b;
    });
    std::vector<uint64_t> sorted((size_t)n * mw);
    for (long long i = 0; i < n; ++i) for (int j = 0; j < mw; ++j) sorted[(size_t)i * mw + j] = masks[(size_t)order[(size_t)i] * mw + j];
    for (long long i = 1; i < n; ++i) {   // two regions with one active set: no unique neighbour, no walk
        bool same = true;
        for (int j = 0; j < mw; ++j) same = same && sorted[(size_t)i * mw + j] == sorted[(size_t)(i - 1) * mw + j];
        if (same) return fail(nullptr, MPC_ERR_INVALID, "mpc_locator_set_adjacency: two regions share one active set");
    }
    hipStream_t st = L->stream;
    HIP_TRY(nullptr, locator_upload(L, L->masks, masks, (size_t)n * mw * sizeof(uint64_t)));
    HIP_TRY(nullptr, locator_upload(L, L->sorted_masks, sorted.data(), (size_t)n * mw * sizeof(uint64_t)));
    HIP_TRY(nullptr, locator_upload(L, L->sorted_region, order.data(), (size_t)n * sizeof(int32_t)));
    HIP_TRY(nullptr, locator_upload(L, L->row_info, row_info, (size_t)rows * sizeof(int32_t)));
    HIP_TRY(nullptr, hipStreamSynchronize(st));
    L->mask_words = mw;
    L->n_c = n_c;
    L->has_adj = true;
    return MPC_OK;
}

// the list scan of k_locate over m points
static void locate_scan(mpc_locator *L, long long m, const double *theta, double tol, int32_t flags, long long *out) {
    const double *Q = L->hasQ ? L->Q.as<double>() : nullptr, *c = L->hasc ? L->c.as<double>() : nullptr, *H = L->hasH ? L->H.as<double>() : nullptr;
    with_width(L->n_t, [&](auto W) {
        hipLaunchKernelGGL((k_locate<decltype(W)::value>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, L->stream, m, L->n_t, L->n_x, L->n_regions, L->n_rows,
                           L->row_region.as<int32_t>(), L->row_end.as<int32_t>(), L->ef.as<double>(), L->xlaw.as<double>(), Q, c, H, theta, tol,
                           (int)(flags & MPC_LOCATE_OVERLAPPING), (int)((flags & MPC_LOCATE_INCLUSIVE) != 0), out);
    });
}

// Behind a tree descent or a walk: fetches region[], locates the points left open (-2) again by the list scan, scatters the
// results into region[] and uploads it again for k_evaluate.  few_ok (the walk): up to 16,384 open points go to k_locate_few.
static int rescan_open(mpc_locator *L, int64_t m, const double *theta, double tol, int32_t flags, bool few_ok, int64_t *region) {
    hipStream_t st = L->stream;
    const int nt = L->n_t;
    HIP_TRY(nullptr, hipMemcpyAsync(region, L->region.p, (size_t)m * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(nullptr, hipStreamSynchronize(st));
    std::vector<long long> open;
    for (long long p = 0; p < m; ++p) if (region[p] == -2) open.push_back(p);
    L->last_unresolved = (long long)open.size();
    if (open.empty()) return MPC_OK;
    const long long mo = (long long)open.size();
    std::vector<double> tho((size_t)mo * nt);
    for (long long i = 0; i < mo; ++i) std::memcpy(&tho[(size_t)i * nt], theta + (size_t)open[(size_t)i] * nt, sizeof(double) * nt);
    std::vector<long long> ro((size_t)mo);
    HIP_TRY(nullptr, L->theta2.ensure((size_t)mo * nt * sizeof(double), st));
    HIP_TRY(nullptr, L->region2.ensure((size_t)mo * sizeof(long long), st));
    HIP_TRY(nullptr, hipMemcpyAsync(L->theta2.p, tho.data(), (size_t)mo * nt * sizeof(double), hipMemcpyHostToDevice, st));
    if (few_ok && mo <= 16384) {
        // few points: every (point, region) pair in parallel, first containing region by atomicMin
        HIP_TRY(nullptr, hipMemsetAsync(L->region2.p, 0xff, (size_t)mo * sizeof(long long), st));   // = "none yet" (max u64)
        const dim3 gf((unsigned)((L->n_regions + 255) / 256), (unsigned)mo);
        with_width(nt, [&](auto W) {
            hipLaunchKernelGGL((k_locate_few<decltype(W)::value>), gf, dim3(256), 0, st, mo, nt, L->n_regions, L->row_off.as<long long>(), L->ef.as<double>(),
                               L->theta2.as<double>(), tol, L->region2.as<long long>());
        });
    } else {
        locate_scan(L, mo, L->theta2.as<double>(), tol, flags, L->region2.as<long long>());
    }
    HIP_TRY(nullptr, hipGetLastError());
    HIP_TRY(nullptr, hipMemcpyAsync(ro.data(), L->region2.p, (size_t)mo * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(nullptr, hipStreamSynchronize(st));
    for (long long i = 0; i < mo; ++i) region[open[(size_t)i]] = ro[(size_t)i];   // -1 (all ones) where no region contains the point
    HIP_TRY(nullptr, hipMemcpyAsync(L->region.p, region, (size_t)m * sizeof(long long), hipMemcpyHostToDevice, st));   // k_evaluate reads it
    return MPC_OK;
}

extern "C" int mpc_locator_query(mpc_locator *L, int64_t m, const double *theta, double tol, int32_t flags, int64_t *region, double *x,
                                 float *ms_locate) {
    if (!L || m < 0 || (m > 0 && (!theta || !region))) return MPC_ERR_INVALID;
    if (ms_locate) *ms_locate = 0.0f;
    const bool tree = (flags & MPC_LOCATE_TREE) != 0;
    if (tree && !L->has_tree) return fail(nullptr, MPC_ERR_INVALID, "mpc_locator_query: MPC_LOCATE_TREE without an attached tree");
    if (tree && !(tol <= L->tree_tol)) return fail(nullptr, MPC_ERR_INVALID, "mpc_locator_query: tol is larger than the tolerance the tree was built for");
    L->last_unresolved = 0;
    if (m == 0) return MPC_OK;
    HIP_TRY(nullptr, hipSetDevice(L->device));
    hipStream_t st = L->stream;
    const int nt = L->n_t, nx = L->n_x;
    HIP_TRY(nullptr, L->theta.ensure((size_t)m * nt * sizeof(double), st));
    HIP_TRY(nullptr, L->region.ensure((size_t)m * sizeof(long long), st));
    HIP_TRY(nullptr, hipMemcpyAsync(L->theta.p, theta, (size_t)m * nt * sizeof(double), hipMemcpyHostToDevice, st));
    const dim3 g((unsigned)((m + 255) / 256)), b(256);
    HIP_TRY(nullptr, hipEventRecord(L->e0, st));
    const bool walk = (flags & MPC_LOCATE_WALK) && L->has_adj && !(flags & (MPC_LOCATE_OVERLAPPING | MPC_LOCATE_INCLUSIVE)) && L->n_regions > 0 && nt <= 16;
    if (tree) {
        // descent of the attached tree; points whose band stack overflowed (-2) go to the list scan
        const double *Q = L->hasQ ? L->Q.as<double>() : nullptr, *c = L->hasc ? L->c.as<double>() : nullptr, *H = L->hasH ? L->H.as<double>() : nullptr;
        with_width(nt, [&](auto W) {
            hipLaunchKernelGGL((k_locate_tree<decltype(W)::value>), g, b, 0, st, (long long)m, nt, nx, L->t_planes.as<double>(), L->t_plane.as<int32_t>(),
                               L->t_child.as<int32_t>(), L->t_tau.as<double>(), L->t_off.as<long long>(), L->t_items.as<int32_t>(),
                               L->row_off.as<long long>(), L->ef.as<double>(), L->xlaw.as<double>(), Q, c, H, L->theta.as<double>(), tol,
                               (int)(flags & MPC_LOCATE_OVERLAPPING), (int)((flags & MPC_LOCATE_INCLUSIVE) != 0), L->region.as<long long>());
        });
        HIP_TRY(nullptr, hipGetLastError());
        if (int rc = rescan_open(L, m, theta, tol, flags, false, region)) return rc;
        HIP_TRY(nullptr, hipEventRecord(L->e1, st));
    } else if (!walk) {
        locate_scan(L, m, L->theta.as<double>(), tol, flags, L->region.as<long long>());
        HIP_TRY(nullptr, hipGetLastError());
        HIP_TRY(nullptr, hipEventRecord(L->e1, st));
        HIP_TRY(nullptr, hipMemcpyAsync(region, L->region.p, (size_t)m * sizeof(long long), hipMemcpyDeviceToHost, st));
    } else {
        // walk through adjacent regions; what the walk cannot resolve goes to the list scan
        const int max_steps = 384;   // walks are tens of steps long; what is still open then (points outside the solution, mostly) goes to k_locate_few
        with_width(nt, [&](auto W) {
            auto launch = [&](auto MW) {
                hipLaunchKernelGGL((k_locate_walk<decltype(W)::value, decltype(MW)::value>), g, b, 0, st, (long long)m, nt, L->n_regions, L->row_off.as<long long>(),
                                   L->ef.as<double>(), L->row_info.as<int32_t>(), L->masks.as<unsigned long long>(), L->sorted_masks.as<unsigned long long>(),
                                   L->sorted_region.as<int32_t>(), L->theta.as<double>(), tol, 0, max_steps, L->n_c, L->region.as<long long>());
            };
            if (L->mask_words == 2) launch(std::integral_constant<int, 2>{}); else launch(std::integral_constant<int, 4>{});
        });
        HIP_TRY(nullptr, hipGetLastError());
        if (int rc = rescan_open(L, m, theta, tol, flags, true, region)) return rc;
        HIP_TRY(nullptr, hipEventRecord(L->e1, st));
    }
    if (x) {
        HIP_TRY(nullptr, L->x.ensure((size_t)m * nx * sizeof(double), st));
        const long long tot = (long long)m * nx;
        hipLaunchKernelGGL(k_evaluate, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (long long)m, nt, nx, L->xlaw.as<double>(), L->theta.as<double>(),
                           L->region.as<long long>(), L->x.as<double>());
        HIP_TRY(nullptr, hipGetLastError());
        HIP_TRY(nullptr, hipMemcpyAsync(x, L->x.p, (size_t)m * nx * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(nullptr, hipStreamSynchronize(st));
    if (ms_locate) HIP_TRY(nullptr, hipEventElapsedTime(ms_locate, L->e0, L->e1));
    return MPC_OK;
}

extern "C" int mpc_locator_last_unresolved(mpc_locator *L, int64_t *n_points) {
    if (!L || !n_points) return MPC_ERR_INVALID;
    *n_points = L->last_unresolved;
    return MPC_OK;
}

// ---- search trees (tree.hpp) ------------------------------------------------------------------------------------
constexpr long long TREE_DEFAULT_BUDGET = 4ll << 30, TREE_MAX_LEVEL_ITEMS = 1ll << 28;

static int tree_attach(mpc_locator *L, int32_t n_planes, const double *planes, int64_t n_nodes, const int32_t *node_plane, const int32_t *node_child,
                       const double *node_tau, const int64_t *node_off, const int32_t *items, double tol) {
    const int nr = L->n_t + 1;
    const int64_t n_items = node_off[n_nodes];
    L->has_tree = false;
    L->h_planes.assign(planes, planes + (size_t)n_planes * nr);
    L->h_plane.assign(node_plane, node_plane + n_nodes);
    L->h_child.assign(node_child, node_child + 2 * n_nodes);
    L->h_tau.assign(node_tau, node_tau + 2 * n_nodes);
    L->h_off.assign(node_off, node_off + n_nodes + 1);
    L->h_items.assign(items, items + n_items);
    hipStream_t st = L->stream;
    HIP_TRY(nullptr, locator_upload(L, L->t_planes, L->h_planes.data(), L->h_planes.size() * 8));
    HIP_TRY(nullptr, locator_upload(L, L->t_plane, L->h_plane.data(), L->h_plane.size() * 4));
    HIP_TRY(nullptr, locator_upload(L, L->t_child, L->h_child.data(), L->h_child.size() * 4));
    HIP_TRY(nullptr, locator_upload(L, L->t_tau, L->h_tau.data(), L->h_tau.size() * 8));
    HIP_TRY(nullptr, locator_upload(L, L->t_off, L->h_off.data(), L->h_off.size() * 8));
    HIP_TRY(nullptr, locator_upload(L, L->t_items, L->h_items.data(), L->h_items.size() * 4));
    HIP_TRY(nullptr, hipStreamSynchronize(st));
    L->tree_planes = n_planes;
    L->tree_tol = tol;
    L->has_tree = true;
    return MPC_OK;
}

extern "C" int mpc_locator_set_tree(mpc_locator *L, int32_t n_planes, const double *planes, int64_t n_nodes, const int32_t *node_plane,
                                    const int32_t *node_child, const double *node_tau, const int64_t *node_off, const int32_t *items, double tol) {
    const char *who = "mpc_locator_set_tree";
    if (!L) return bad(who, "no locator");
    if (n_planes < 0 || (n_planes > 0 && !planes)) return bad(who, "bad planes");
    if (n_nodes < 1 || !node_plane || !node_child || !node_tau || !node_off) return bad(who, "missing node arrays");
    if (!std::isfinite(tol) || tol < 0.0) return bad(who, "tol must be finite and >= 0");
    if (node_off[0] != 0) return bad(who, "node_off[0] must be 0");
    const int nr = L->n_t + 1;
    for (int64_t i = 0; i < (int64_t)n_planes * nr; ++i) if (!std::isfinite(planes[i])) return bad(who, "planes must be finite");
    for (int64_t k = 0; k < n_nodes; ++k) {
        if (node_off[k + 1] < node_off[k]) return bad(who, "node_off decreases");
        const int32_t h = node_plane[k];
        if (h < -1 || h >= n_planes) return bad(who, "a node plane is out of range");
        if (h >= 0) {
            for (int q = 0; q < 2; ++q) {
                const int32_t ch = node_child[2 * k + q];
                if (ch <= k || ch >= n_nodes) return bad(who, "a child index is not after its parent or out of range");
                if (!(node_tau[2 * k + q] >= 0.0)) return bad(who, "tau must be >= 0");
            }
        }
    }
    if (node_off[n_nodes] > 0 && !items) return bad(who, "missing items");
    for (int64_t k = 0; k < n_nodes; ++k)
        for (int64_t i = node_off[k]; i < node_off[k + 1]; ++i) {
            if (items[i] < 0 || items[i] >= L->n_regions) return bad(who, "a leaf item is not a region index");
            if (i > node_off[k] && items[i] < items[i - 1]) return bad(who, "a leaf list is not ascending");
        }
    HIP_TRY(nullptr, hipSetDevice(L->device));
    return tree_attach(L, n_planes, planes, n_nodes, node_plane, node_child, node_tau, node_off, items, tol);
}

extern "C" int mpc_locator_tree_size(mpc_locator *L, int64_t *n_nodes, int64_t *n_items, int32_t *n_planes, double *tol) {
    if (!L || !L->has_tree) return fail(nullptr, MPC_ERR_INVALID, "mpc_locator_tree_size: no tree attached");
    if (n_nodes) *n_nodes = (int64_t)L->h_plane.size();
    if (n_items) *n_items = (int64_t)L->h_items.size();
    if (n_planes) *n_planes = L->tree_planes;
    if (tol) *tol = L->tree_tol;
    return MPC_OK;
}

extern "C" int mpc_locator_get_tree(mpc_locator *L, double *planes, int32_t *node_plane, int32_t *node_child, double *node_tau, int64_t *node_off,
                                    int32_t *items) {
    if (!L || !L->has_tree) return fail(nullptr, MPC_ERR_INVALID, "mpc_locator_get_tree: no tree attached");
    auto put = [](void *dst, const auto &v) { if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
    put(planes, L->h_planes); put(node_plane, L->h_plane); put(node_child, L->h_child); put(node_tau, L->h_tau); put(node_off, L->h_off);
    put(items, L->h_items);
    return MPC_OK;
}

extern "C" int mpc_tree_build(mpc_locator *L, int32_t n_planes, const double *planes, const int64_t *cand_off, const int32_t *cand_plane, double tol,
                              double band, int32_t leaf_size, int32_t max_depth, int64_t budget, mpc_tree_stats *stats) {
    const auto t_start = std::chrono::steady_clock::now();
    const char *who = "mpc_tree_build";
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (!L) return bad(who, "no locator");
    const int nt = L->n_t, nr = nt + 1;
    const long long R = L->n_regions;
    if (nt < 1 || nt > TR_MAX_NT) return bad(who, "n_t must lie in 1..16");
    if (n_planes < 0 || (n_planes > 0 && !planes)) return bad(who, "bad planes");
    if (!std::isfinite(tol) || tol < 0.0) return bad(who, "tol must be finite and >= 0");
    if (!std::isfinite(band) || band < 0.0) return bad(who, "band must be finite and >= 0");
    if (leaf_size < 1) return bad(who, "leaf_size must be >= 1");
    if (max_depth < 1 || max_depth > 64) return bad(who, "max_depth must lie in 1..64");
    if ((cand_off == nullptr) != (cand_plane == nullptr)) return bad(who, "cand_off and cand_plane go together");
    int m_max = 0;
    for (long long r = 0; r < R; ++r) {
        const long long k = L->h_row_off[(size_t)r + 1] - L->h_row_off[(size_t)r];
        if (k > TR_MAX_ROWS) return bad(who, "a region has more than 256 rows");
        m_max = std::max<int>(m_max, (int)k);
    }
    for (int h = 0; h < n_planes; ++h) {
        double nn = 0.0;
        for (int t = 0; t < nt; ++t) nn += planes[(size_t)h * nr + t] * planes[(size_t)h * nr + t];
        if (!std::isfinite(planes[(size_t)h * nr + nt]) || !(std::fabs(std::sqrt(nn) - 1.0) <= 1e-6)) return bad(who, "planes must be finite with unit normals");
    }
    if (cand_off) {
        if (cand_off[0] != 0) return bad(who, "cand_off[0] must be 0");
        for (long long r = 0; r < R; ++r) if (cand_off[r + 1] < cand_off[r]) return bad(who, "cand_off decreases");
        for (long long i = 0; i < cand_off[R]; ++i) if (cand_plane[i] < 0 || cand_plane[i] >= n_planes) return bad(who, "a candidate plane is out of range");
    }
    const int hw = (n_planes + 63) / 64;
    const long long limit = budget > 0 ? budget : TREE_DEFAULT_BUDGET;
    const long long bitset_bytes = (cand_off ? 3 : 2) * (long long)R * hw * 8;
    if (bitset_bytes > limit) {
        char msg[200];
        snprintf(msg, sizeof msg, "the classification bitsets need %lld bytes, over the budget of %lld bytes", bitset_bytes, limit);
        return bad(who, msg);
    }
    HIP_TRY(nullptr, hipSetDevice(L->device));
    hipStream_t st = L->stream;
    OneShot s(who, st, true);   // owns the buffers and the two events on every way out, the early returns of HIP_TRY included
    if (!s.ok()) return s.finish();
    DevBuf &d_planes = s.buf(), &d_plus = s.buf(), &d_minus = s.buf(), &d_owner = s.buf(), &d_xs = s.buf(), &d_empty = s.buf(), &d_cnt = s.buf(),
           &d_items = s.buf(), &d_off = s.buf(), &d_part = s.buf(), &d_iplane = s.buf(), &d_side = s.buf(), &d_pairs = s.buf(), &d_nplane = s.buf(),
           &d_tau = s.buf(), &d_er = s.buf(), &d_ep = s.buf();
    float ms_classify = 0.0f, ms_split = 0.0f, ms_tau = 0.0f;
    auto timed = [&](float &acc, auto &&launch) -> hipError_t {
        hipError_t e = hipEventRecord(s.e0, st);
        if (e != hipSuccess) return e;
        launch();
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipEventRecord(s.e1, st)) != hipSuccess) return e;
        if ((e = hipEventSynchronize(s.e1)) != hipSuccess) return e;
        float ms = 0.0f;
        if ((e = hipEventElapsedTime(&ms, s.e0, s.e1)) != hipSuccess) return e;
        acc += ms;
        return hipSuccess;
    };
    unsigned long long cnt[5] = {0, 0, 0, 0, 0};
    HIP_TRY(nullptr, locator_upload(L, d_cnt, cnt, sizeof cnt));
    TreeClassifyArgs a{};
    a.nt = nt; a.m_max = std::max(m_max, 1); a.n_planes = n_planes; a.hw = hw; a.n_regions = R;
    a.row_off = L->row_off.as<long long>(); a.ef = L->ef.as<double>(); a.tol = tol; a.band = band;
    a.counters = d_cnt.as<unsigned long long>();
    const size_t lds = tr_lds_bytes(a.m_max, nt);
    if (R > 0 && n_planes > 0) {
        HIP_TRY(nullptr, locator_upload(L, d_planes, planes, (size_t)n_planes * nr * 8));
        const size_t bits = (size_t)R * hw * 8;
        HIP_TRY(nullptr, d_plus.ensure(bits, st)); HIP_TRY(nullptr, d_minus.ensure(bits, st));
        HIP_TRY(nullptr, hipMemsetAsync(d_plus.p, 0, bits, st)); HIP_TRY(nullptr, hipMemsetAsync(d_minus.p, 0, bits, st));
        HIP_TRY(nullptr, d_xs.ensure((size_t)R * nt * 8, st)); HIP_TRY(nullptr, d_empty.ensure((size_t)R * 4, st));
        if (cand_off && cand_off[R] > 0) {
            HIP_TRY(nullptr, d_owner.ensure(bits, st));
            HIP_TRY(nullptr, hipMemsetAsync(d_owner.p, 0, bits, st));
            std::vector<int32_t> er((size_t)cand_off[R]);
            for (long long r = 0; r < R; ++r) for (long long i = cand_off[r]; i < cand_off[r + 1]; ++i) er[(size_t)i] = (int32_t)r;
            HIP_TRY(nullptr, locator_upload(L, d_er, er.data(), er.size() * 4));
            HIP_TRY(nullptr, locator_upload(L, d_ep, cand_plane, er.size() * 4));
            const long long ne = cand_off[R];
            hipLaunchKernelGGL(k_tree_owner, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, ne, hw, d_er.as<int32_t>(), d_ep.as<int32_t>(),
                               d_owner.as<unsigned long long>());
            HIP_TRY(nullptr, hipGetLastError());
        }
        a.planes = d_planes.as<double>(); a.plus = d_plus.as<unsigned long long>(); a.minus = d_minus.as<unsigned long long>();
        a.xs = d_xs.as<double>(); a.empty = d_empty.as<int32_t>();
        HIP_TRY(nullptr, timed(ms_classify, [&] { hipLaunchKernelGGL((k_tree_classify<0>), dim3((unsigned)R), dim3(64), lds, st, a); }));
    }
    const unsigned long long *owner = (cand_off && cand_off[R] > 0) ? d_owner.as<unsigned long long>() : nullptr;
    // the level loop: host node records, device counts
    struct Node { int32_t plane = -1, child[2] = {-1, -1}; double tau[2] = {0.0, 0.0}; int depth = 0; std::vector<int32_t> list; };
    std::vector<Node> nodes(1);
    nodes[0].list.resize((size_t)R);
    for (long long r = 0; r < R; ++r) nodes[0].list[(size_t)r] = (int32_t)r;
    std::vector<int> level{0};
    long long tau_lps = 0;
    while (!level.empty() && n_planes > 0) {
        std::vector<int> work;
        for (int k : level) if ((long long)nodes[k].list.size() > leaf_size && nodes[k].depth < max_depth) work.push_back(k);
        if (work.empty()) break;
        std::vector<long long> off(work.size() + 1, 0);
        for (size_t w = 0; w < work.size(); ++w) off[w + 1] = off[w] + (long long)nodes[work[w]].list.size();
        if (off.back() > TREE_MAX_LEVEL_ITEMS) return fail(nullptr, MPC_ERR_CAPACITY, "mpc_tree_build: a level holds more than 2^28 (node, region) entries");
        std::vector<int32_t> items((size_t)off.back());
        for (size_t w = 0; w < work.size(); ++w) std::copy(nodes[work[w]].list.begin(), nodes[work[w]].list.end(), items.begin() + off[w]);
        HIP_TRY(nullptr, locator_upload(L, d_items, items.data(), items.size() * 4));
        HIP_TRY(nullptr, locator_upload(L, d_off, off.data(), off.size() * 8));
        const long long nw = (long long)work.size();
        const long long target_chunks = std::max<long long>(1, 4096 / nw);
        const int chunk_len = (int)std::max<long long>(TS_BLOCK, (((n_planes + target_chunks - 1) / target_chunks) + TS_BLOCK - 1) / TS_BLOCK * TS_BLOCK);
        const int chunks = (n_planes + chunk_len - 1) / chunk_len;
        HIP_TRY(nullptr, d_part.ensure((size_t)nw * chunks * sizeof(int4), st));
        HIP_TRY(nullptr, timed(ms_split, [&] {
            hipLaunchKernelGGL(k_tree_split, dim3((unsigned)nw, (unsigned)chunks), dim3(TS_BLOCK), 0, st, n_planes, hw, chunk_len, d_off.as<long long>(),
                               d_items.as<int32_t>(), d_plus.as<unsigned long long>(), d_minus.as<unsigned long long>(), owner, d_part.as<int4>());
        }));
        std::vector<int4> part((size_t)nw * chunks);
        HIP_TRY(nullptr, hipMemcpy(part.data(), d_part.p, part.size() * sizeof(int4), hipMemcpyDeviceToHost));
        std::vector<int32_t> item_plane(items.size(), 0);
        std::vector<int> inner;
        for (long long w = 0; w < nw; ++w) {
            int bmx = TS_NONE, bn0 = TS_NONE, bh = -1;
            for (int c = 0; c < chunks; ++c) {
                const int4 q = part[(size_t)(w * chunks + c)];
                if (q.z < 0) continue;
                if (bh < 0 || q.x < bmx || (q.x == bmx && (q.y < bn0 || (q.y == bn0 && q.z < bh)))) { bmx = q.x; bn0 = q.y; bh = q.z; }
            }
            Node &nd = nodes[work[(size_t)w]];
            if (bh < 0 || bmx >= (int)nd.list.size()) continue;   // no plane makes progress: a leaf
            nd.plane = bh;
            inner.push_back((int)w);
            std::fill(item_plane.begin() + off[w], item_plane.begin() + off[w + 1], bh);
        }
        if (inner.empty()) break;
        HIP_TRY(nullptr, locator_upload(L, d_iplane, item_plane.data(), item_plane.size() * 4));
        HIP_TRY(nullptr, d_side.ensure(items.size(), st));
        HIP_TRY(nullptr, timed(ms_split, [&] {
            hipLaunchKernelGGL(k_tree_partition, dim3((unsigned)((items.size() + 255) / 256)), dim3(256), 0, st, (long long)items.size(), hw,
                               d_items.as<int32_t>(), d_iplane.as<int32_t>(), d_plus.as<unsigned long long>(), d_minus.as<unsigned long long>(),
                               d_side.as<int8_t>());
        }));
        std::vector<int8_t> side(items.size());
        HIP_TRY(nullptr, hipMemcpy(side.data(), d_side.p, side.size(), hipMemcpyDeviceToHost));
        // children and the one-sided (node, region) pairs of tau
        std::vector<int32_t> pairs, nplane;
        std::vector<int> next;
        for (size_t q = 0; q < inner.size(); ++q) {
            const long long w = inner[q];
            const int k = work[(size_t)w];
            Node cp, cm;
            cp.depth = cm.depth = nodes[k].depth + 1;
            for (long long i = off[w]; i < off[w + 1]; ++i) {
                const int32_t j = items[(size_t)i];
                const int sd = side[(size_t)i];
                if (sd != 2) cp.list.push_back(j);
                if (sd != 1) cm.list.push_back(j);
                if (sd) { pairs.push_back((int32_t)q); pairs.push_back(j); pairs.push_back(sd - 1); }
            }
            nplane.push_back(nodes[k].plane);
            const int ip = (int)nodes.size();
            nodes[k].child[0] = ip; nodes[k].child[1] = ip + 1;
            nodes[k].list.clear(); nodes[k].list.shrink_to_fit();
            nodes.push_back(std::move(cp)); nodes.push_back(std::move(cm));
            next.push_back(ip); next.push_back(ip + 1);
        }
        const long long n_pairs = (long long)pairs.size() / 3;
        std::vector<unsigned long long> tau(2 * inner.size(), 0ull);
        if (n_pairs > 0) {
            HIP_TRY(nullptr, locator_upload(L, d_pairs, pairs.data(), pairs.size() * 4));
            HIP_TRY(nullptr, locator_upload(L, d_nplane, nplane.data(), nplane.size() * 4));
            HIP_TRY(nullptr, locator_upload(L, d_tau, tau.data(), tau.size() * 8));
            TreeClassifyArgs b = a;
            b.n_pairs = n_pairs; b.pair = d_pairs.as<int32_t>(); b.node_plane = d_nplane.as<int32_t>(); b.tau = d_tau.as<unsigned long long>();
            HIP_TRY(nullptr, timed(ms_tau, [&] { hipLaunchKernelGGL((k_tree_classify<1>), dim3((unsigned)n_pairs), dim3(64), lds, st, b); }));
            HIP_TRY(nullptr, hipMemcpy(tau.data(), d_tau.p, tau.size() * 8, hipMemcpyDeviceToHost));
            tau_lps += n_pairs;
        }
        for (size_t q = 0; q < inner.size(); ++q) {
            Node &nd = nodes[work[(size_t)inner[q]]];
            for (int sd = 0; sd < 2; ++sd) { double v; std::memcpy(&v, &tau[2 * q + sd], 8); nd.tau[sd] = v; }
        }
        level.swap(next);
    }
    HIP_TRY(nullptr, hipMemcpy(cnt, d_cnt.p, sizeof cnt, hipMemcpyDeviceToHost));
    // flatten
    const int64_t N = (int64_t)nodes.size();
    std::vector<int32_t> plane_v((size_t)N), child_v((size_t)(2 * N)), items_v;
    std::vector<double> tau_v((size_t)(2 * N));
    std::vector<int64_t> off_v((size_t)N + 1, 0);
    int64_t n_leaves = 0, max_leaf = 0, depth = 0;
    for (int64_t k = 0; k < N; ++k) {
        const Node &nd = nodes[(size_t)k];
        plane_v[(size_t)k] = nd.plane;
        for (int q = 0; q < 2; ++q) { child_v[(size_t)(2 * k + q)] = nd.child[q]; tau_v[(size_t)(2 * k + q)] = nd.tau[q]; }
        if (nd.plane < 0) {
            items_v.insert(items_v.end(), nd.list.begin(), nd.list.end());
            ++n_leaves;
            max_leaf = std::max<int64_t>(max_leaf, (int64_t)nd.list.size());
        }
        off_v[(size_t)k + 1] = (int64_t)items_v.size();
        depth = std::max<int64_t>(depth, nd.depth);
    }
    if (int rc = tree_attach(L, n_planes, planes, N, plane_v.data(), child_v.data(), tau_v.data(), off_v.data(), items_v.data(), tol)) return rc;
    if (stats) {
        stats->n_nodes = N; stats->n_leaves = n_leaves; stats->depth = depth; stats->max_leaf = max_leaf;
        stats->leaf_items = (int64_t)items_v.size();
        stats->mean_leaf = n_leaves ? (double)items_v.size() / (double)n_leaves : 0.0;
        stats->pairs = (int64_t)cnt[0]; stats->box_pairs = (int64_t)cnt[1]; stats->lps = (int64_t)cnt[2]; stats->pivots = (int64_t)cnt[3];
        stats->capped = (int64_t)cnt[4]; stats->tau_lps = tau_lps; stats->bitset_bytes = bitset_bytes;
        stats->ms_classify = ms_classify; stats->ms_split = ms_split; stats->ms_tau = ms_tau;
        stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    return MPC_OK;
}

extern "C" int mpc_locator_destroy(mpc_locator *L) {
    if (!L) return MPC_OK;
    (void)hipSetDevice(L->device);
    if (L->stream) (void)hipStreamSynchronize(L->stream);
    for (DevBuf *b : {&L->row_off, &L->row_region, &L->row_end, &L->ef, &L->xlaw, &L->Q, &L->c, &L->H, &L->theta, &L->region, &L->x, &L->masks, &L->sorted_masks,
                      &L->sorted_region, &L->row_info, &L->theta2, &L->region2, &L->t_planes, &L->t_plane, &L->t_child, &L->t_tau, &L->t_off,
                      &L->t_items}) b->release();
    if (L->e0) (void)hipEventDestroy(L->e0);
    if (L->e1) (void)hipEventDestroy(L->e1);
    if (L->stream) (void)hipStreamDestroy(L->stream);
    delete L;
    return MPC_OK;
}

// ---- closed-loop simulation (closed_loop.hpp) --------------------------------------------------------------------------
constexpr long long SIM_DEFAULT_BUDGET = 4ll << 30;

extern "C" int mpc_locator_simulate(mpc_locator *L, int64_t n, int32_t steps, const double *theta0, int32_t n_u, const int32_t *inputs,
                                    const double *A, const double *B, const double *c, const double *w, const double *box_lo,
                                    const double *box_hi, uint64_t seed, double tol, double stop_tol, int32_t flags, int64_t budget,
                                    double *theta, double *u, int32_t *region, int32_t *status, int32_t *exit_step, mpc_sim_stats *stats) {
    const char *who = "mpc_locator_simulate";
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (!L) return bad(who, "no locator");
    const int nt = L->n_t, nx = L->n_x;
    const bool final_only = (flags & MPC_SIM_FINAL) != 0, tree = (flags & MPC_LOCATE_TREE) != 0, walk = (flags & MPC_LOCATE_WALK) != 0;
    const bool overlapping = (flags & MPC_LOCATE_OVERLAPPING) != 0, inclusive = (flags & MPC_LOCATE_INCLUSIVE) != 0;
    if (n < 0 || n > (1ll << 40) || steps < 1 || steps > (1 << 30)) return bad(who, "n must lie in 0..2^40 and steps in 1..2^30");
    if (nt < 1 || nt > 16) return bad(who, "n_theta must lie in 1..16");
    if (n_u < 1 || n_u > 16) return bad(who, "n_u must lie in 1..16");
    if (L->n_regions < 1) return bad(who, "the locator holds no region");
    if (n > 0 && (!theta0 || !theta || !status || !exit_step)) return bad(who, "missing theta0, theta, status or exit_step");
    if (n > 0 && !final_only && (!u || !region)) return bad(who, "a full record needs u and region");
    if (!inputs || !A || !B) return bad(who, "missing inputs, A or B");
    for (int i = 0; i < n_u; ++i)
        if (inputs[i] < 0 || inputs[i] >= nx) return bad(who, "input index " + std::to_string(inputs[i]) + " is out of range (0 <= inputs < n_x = " + std::to_string(nx) + ")");
    auto finite = [](const double *v, long long k) { for (long long i = 0; i < k; ++i) if (!std::isfinite(v[i])) return false; return true; };
    if (!finite(A, (long long)nt * nt) || !finite(B, (long long)nt * n_u) || (c && !finite(c, nt))) return bad(who, "A, B and c must be finite");
    if (n > 0 && !finite(theta0, n * nt)) return bad(who, "theta0 must be finite");
    if (w && (box_lo || box_hi)) return bad(who, "a disturbance array and a box exclude each other");
    if ((box_lo == nullptr) != (box_hi == nullptr)) return bad(who, "box_lo and box_hi go together");
    if (box_lo)
        for (int t = 0; t < nt; ++t)
            if (!std::isfinite(box_lo[t]) || !std::isfinite(box_hi[t]) || !(box_lo[t] <= box_hi[t])) return bad(who, "the box must be finite with lo <= hi");
    if (w && n > 0 && !finite(w, n * (long long)steps * nt)) return bad(who, "the disturbance must be finite");
    if (!std::isfinite(tol) || tol < 0.0) return bad(who, "tol must be finite and >= 0");
    if (std::isnan(stop_tol)) return bad(who, "stop_tol must not be NaN (< 0: off)");
    if (tree && walk) return bad(who, "MPC_LOCATE_TREE and MPC_LOCATE_WALK exclude each other");
    if (tree && !L->has_tree) return bad(who, "MPC_LOCATE_TREE without an attached tree");
    if (tree && !(tol <= L->tree_tol)) return bad(who, "tol is larger than the tolerance the tree was built for");
    if (walk && (!L->has_adj || overlapping || inclusive)) return bad(who, "MPC_LOCATE_WALK needs adjacency, and neither MPC_LOCATE_OVERLAPPING nor MPC_LOCATE_INCLUSIVE");
    // device bytes of the record and the inputs (doubles: no overflow for any n, steps that pass above)
    const double rec = final_only ? (double)n * nt * 8 : (double)n * ((double)(steps + 1) * nt * 8 + (double)steps * (n_u * 8 + 4));
    const double bytes = rec + (double)n * nt * 8 + (w ? (double)n * steps * nt * 8 : 0.0);
    const double cap = budget > 0 ? (double)budget : (double)SIM_DEFAULT_BUDGET;
    if (bytes > cap)
        return bad(who, "the run needs " + std::to_string((long long)bytes) + " device bytes, more than the budget of " + std::to_string((long long)cap) +
                   " (record the final states only, or run fewer trajectories at a time)");
    if (n == 0) return MPC_OK;
    HIP_TRY(nullptr, hipSetDevice(L->device));
    hipStream_t st = L->stream;
    const size_t n_th = (size_t)(final_only ? 1 : steps + 1) * n * nt, n_uu = final_only ? 0 : (size_t)steps * n * n_u, n_rg = final_only ? 0 : (size_t)steps * n;
    // the plant in one block: A [nt][nt], B [nt][n_u], c [nt], lo [nt], hi [nt], then the inputs
    std::vector<double> plant((size_t)nt * nt + (size_t)nt * n_u + 3 * (size_t)nt, 0.0);
    std::memcpy(plant.data(), A, sizeof(double) * nt * nt);
    std::memcpy(plant.data() + nt * nt, B, sizeof(double) * nt * n_u);
    const size_t oc = (size_t)nt * nt + (size_t)nt * n_u, olo = oc + nt, ohi = olo + nt;
    if (c) std::memcpy(plant.data() + oc, c, sizeof(double) * nt);
    if (box_lo) { std::memcpy(plant.data() + olo, box_lo, sizeof(double) * nt); std::memcpy(plant.data() + ohi, box_hi, sizeof(double) * nt); }
    unsigned long long cnt[3] = {0, 0, 0};
    float ms = 0.0f;
    OneShot s(who, st);
    DevBuf &d_th0 = s.upload(theta0, (size_t)n * nt * 8);
    DevBuf &d_w = w ? s.upload(w, (size_t)n * steps * nt * 8) : s.buf();
    DevBuf &d_plant = s.upload(plant.data(), plant.size() * 8), &d_in = s.upload(inputs, (size_t)n_u * 4);
    DevBuf &d_cnt = s.buf(3 * 8), &d_th = s.buf(n_th * 8), &d_u = s.buf(n_uu * 8), &d_rg = s.buf(n_rg * 4);
    DevBuf &d_st = s.buf((size_t)n * 4), &d_ex = s.buf((size_t)n * 4);
    s.fill(d_cnt, 0, 3 * 8);
    if (!final_only) {   // what lies after a trajectory's end is never written: NaN (all bits set) and region -1
        s.fill(d_th, 0xff, n_th * 8);
        s.fill(d_u, 0xff, n_uu * 8);
        s.fill(d_rg, 0xff, n_rg * 4);
    }
    const double *pl = d_plant.as<double>();
    SimArgs a{};
    a.n = n; a.steps = steps; a.nt = nt; a.nx = nx; a.nu = n_u;
    a.n_regions = L->n_regions; a.n_rows = L->n_rows;
    a.row_off = L->row_off.as<long long>(); a.row_region = L->row_region.as<int32_t>(); a.row_end = L->row_end.as<int32_t>();
    a.ef = L->ef.as<double>(); a.xlaw = L->xlaw.as<double>();
    a.Q = L->hasQ ? L->Q.as<double>() : nullptr; a.cvec = L->hasc ? L->c.as<double>() : nullptr; a.H = L->hasH ? L->H.as<double>() : nullptr;
    a.tol = tol; a.overlapping = overlapping; a.inclusive = inclusive;
    if (walk) {
        a.row_info = L->row_info.as<int32_t>(); a.sorted_region = L->sorted_region.as<int32_t>();
        a.masks = L->masks.as<unsigned long long>(); a.sorted_masks = L->sorted_masks.as<unsigned long long>();
        a.n_c = L->n_c; a.max_walk = 384;   // the step limit of mpc_locator_query's walk
    }
    if (tree) {
        a.planes = L->t_planes.as<double>(); a.node_tau = L->t_tau.as<double>(); a.node_plane = L->t_plane.as<int32_t>();
        a.node_child = L->t_child.as<int32_t>(); a.items = L->t_items.as<int32_t>(); a.node_off = L->t_off.as<long long>();
    }
    a.theta0 = d_th0.as<double>(); a.inputs = d_in.as<int32_t>();
    a.A = pl; a.B = pl + nt * nt; a.c = c ? pl + oc : nullptr; a.w = w ? d_w.as<double>() : nullptr;
    a.lo = box_lo ? pl + olo : nullptr; a.hi = box_lo ? pl + ohi : nullptr;
    a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32) ^ MPC_SIM_KEY_SALT;
    a.stop_tol = stop_tol; a.final_only = final_only;
    a.theta = d_th.as<double>(); a.u = final_only ? nullptr : d_u.as<double>(); a.region = final_only ? nullptr : d_rg.as<int32_t>();
    a.status = d_st.as<int32_t>(); a.exit_step = d_ex.as<int32_t>(); a.counters = d_cnt.as<unsigned long long>();
    const dim3 g((unsigned)((n + SIM_BLOCK - 1) / SIM_BLOCK)), b(SIM_BLOCK);
    // k_simulate<width of theta, width of u (4 | 16), mode>
    auto launch = [&](auto MODE) {
        with_width(nt, [&](auto W) {
            if (n_u <= 4) hipLaunchKernelGGL((k_simulate<decltype(W)::value, 4, decltype(MODE)::value>), g, b, 0, st, a);
            else hipLaunchKernelGGL((k_simulate<decltype(W)::value, 16, decltype(MODE)::value>), g, b, 0, st, a);
        });
    };
    if (s.ok()) s.chk(hipEventRecord(L->e0, st));
    s.launch([&] {
        if (tree) launch(std::integral_constant<int, SIM_TREE>{});
        else if (walk && L->mask_words == 2) launch(std::integral_constant<int, SIM_WALK2>{});
        else if (walk) launch(std::integral_constant<int, SIM_WALK4>{});
        else launch(std::integral_constant<int, SIM_SCAN>{});
    });
    if (s.ok()) s.chk(hipEventRecord(L->e1, st));
    s.download(theta, d_th, n_th * 8);
    s.download(u, d_u, n_uu * 8);        // nothing when only the final states are recorded
    s.download(region, d_rg, n_rg * 4);
    s.download(status, d_st, (size_t)n * 4);
    s.download(exit_step, d_ex, (size_t)n * 4);
    s.download(cnt, d_cnt, 3 * 8);
    s.sync();   // the call's only wait: finish() does not repeat it
    if (s.ok()) s.chk(hipEventElapsedTime(&ms, L->e0, L->e1));
    if (int rc = s.finish()) return rc;
    if (stats) {
        stats->traj_steps = (int64_t)cnt[0]; stats->crossings = (int64_t)cnt[1]; stats->fallbacks = (int64_t)cnt[2];
        stats->mode = tree ? MPC_LOCATE_TREE : walk ? MPC_LOCATE_WALK : 0;
        stats->ms = ms;
    }
    return MPC_OK;
}

// ---- vertex enumeration of a batch of polytopes (vertices.hpp) ---------------------------------------------------------
constexpr long long VX_DEFAULT_BUDGET = 4ll << 30, VX_DEFAULT_SLAB = 256, VX_MAX_SLAB = 1ll << 24;

// device bytes of one polytope's slab: two lists of generators (y, Z), the products s and the two index lists
template <int NT> static double vx_slab_bytes(long long cap) { return (double)cap * (2.0 * (NT + 1) * 8 + 2.0 * VX_MW * 8 + 8 + 2 * 4); }

template <int NT>
static int vx_run(const char *who, int nt, int64_t n_poly, const int64_t *row_off, const double *ef_rows, double tol, long long cap, long long max_slab,
                  double budget, std::vector<int32_t> &status, std::vector<int64_t> &nv, std::vector<int64_t> &nr,
                  std::vector<std::vector<double>> &hv, std::vector<std::vector<uint64_t>> &hz, std::vector<std::vector<double>> &hr,
                  mpc_vertex_stats &stats) {
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_poly, row_off, ef_rows, nt + 1);
    DevBuf &d_poly = s.buf(), &d_y = s.buf(), &d_z = s.buf(), &d_s = s.buf(), &d_i = s.buf(), &d_st = s.buf(), &d_nv = s.buf(), &d_nr = s.buf(),
           &d_buf = s.buf(), &d_cnt = s.buf(), &d_vo = s.buf(), &d_ro = s.buf(), &d_ov = s.buf(), &d_oz = s.buf(), &d_or = s.buf();
    std::vector<int32_t> pending(n_poly);
    for (int64_t p = 0; p < n_poly; ++p) pending[p] = (int32_t)p;
    for (;;) {
        const double per = vx_slab_bytes<NT>(cap);
        const long long chunk = std::max(1ll, std::min<long long>({(long long)pending.size(), (long long)(budget / per), 1ll << 16}));
        std::vector<int32_t> over;
        for (size_t start = 0; start < pending.size(); start += (size_t)chunk) {
            const long long nq = std::min<long long>(chunk, (long long)(pending.size() - start));
            s.upload(d_poly, pending.data() + start, (size_t)nq * 4);
            s.ensure(d_y, (size_t)nq * 2 * cap * (NT + 1) * 8);
            s.ensure(d_z, (size_t)nq * 2 * cap * VX_MW * 8);
            s.ensure(d_s, (size_t)nq * cap * 8);
            s.ensure(d_i, (size_t)nq * 2 * cap * 4);
            for (DevBuf *b : {&d_st, &d_nv, &d_nr, &d_buf}) s.ensure(*b, (size_t)nq * 4);
            s.ensure(d_cnt, (size_t)nq * 3 * 8);
            VxArgs a{};
            a.nt = nt; a.n = nq; a.poly = d_poly.as<int32_t>(); a.row_off = d.off.as<long long>(); a.ef = d.ef.as<double>(); a.cap = cap;
            a.slab_y = d_y.as<double>(); a.slab_z = d_z.as<unsigned long long>(); a.slab_s = d_s.as<double>(); a.slab_i = d_i.as<int32_t>();
            a.tol = tol; a.status = d_st.as<int32_t>(); a.n_vert = d_nv.as<int32_t>(); a.n_ray = d_nr.as<int32_t>(); a.buf = d_buf.as<int32_t>();
            a.counters = d_cnt.as<unsigned long long>();
            s.launch_timed([&] { hipLaunchKernelGGL((k_region_vertices<NT>), dim3((unsigned)nq), dim3(VX_BLOCK), 0, nullptr, a); });
            std::vector<int32_t> st(nq), cv(nq), cr(nq), cb(nq);
            std::vector<unsigned long long> cnt((size_t)nq * 3);
            s.download(st.data(), d_st, (size_t)nq * 4);
            s.download(cv.data(), d_nv, (size_t)nq * 4);
            s.download(cr.data(), d_nr, (size_t)nq * 4);
            s.download(cnt.data(), d_cnt, (size_t)nq * 3 * 8);
            float ms = 0.0f;
            s.elapsed(&ms);
            if (!s.ok()) return s.finish();
            stats.ms += ms;
            stats.launches += 1;
            std::vector<long long> vo(nq), ro(nq);
            long long tv = 0, tr = 0;
            for (long long i = 0; i < nq; ++i) {
                const int32_t p = pending[start + i];
                stats.generators += (int64_t)cnt[i * 3 + 0];
                stats.max_list = std::max<int64_t>(stats.max_list, (int64_t)cnt[i * 3 + 1]);
                stats.merges += (int64_t)cnt[i * 3 + 2];
                status[p] = st[i];
                if (st[i] == VX_OVERFLOW) { over.push_back(p); cv[i] = cr[i] = 0; }
                nv[p] = cv[i]; nr[p] = cr[i];
                vo[i] = tv; ro[i] = tr;
                tv += cv[i]; tr += cr[i];
            }
            if (tv + tr == 0) continue;
            // pack this launch's results (the counts of overflowed polytopes are 0 on the device too)
            s.upload(d_vo, vo.data(), (size_t)nq * 8);
            s.upload(d_ro, ro.data(), (size_t)nq * 8);
            s.ensure(d_ov, std::max<size_t>(8, (size_t)tv * nt * 8));
            s.ensure(d_oz, std::max<size_t>(8, (size_t)tv * VX_OUT_MW * 8));
            s.ensure(d_or, std::max<size_t>(8, (size_t)tr * nt * 8));
            s.launch([&] {
                hipLaunchKernelGGL((k_vertices_gather<NT>), dim3((unsigned)nq), dim3(VX_BLOCK), 0, nullptr, nt, cap, d_y.as<double>(),
                                   d_z.as<unsigned long long>(), d_nv.as<int32_t>(), d_nr.as<int32_t>(), d_buf.as<int32_t>(), d_vo.as<long long>(),
                                   d_ro.as<long long>(), d_ov.as<double>(), d_oz.as<unsigned long long>(), d_or.as<double>());
            });
            std::vector<double> ov((size_t)tv * nt), orr((size_t)tr * nt);
            std::vector<uint64_t> oz((size_t)tv * VX_OUT_MW);
            s.download(ov.data(), d_ov, ov.size() * 8);
            s.download(oz.data(), d_oz, oz.size() * 8);
            s.download(orr.data(), d_or, orr.size() * 8);
            if (!s.ok()) return s.finish();
            for (long long i = 0; i < nq; ++i) {
                const int32_t p = pending[start + i];
                hv[p].assign(ov.begin() + vo[i] * nt, ov.begin() + (vo[i] + cv[i]) * nt);
                hz[p].assign(oz.begin() + vo[i] * VX_OUT_MW, oz.begin() + (vo[i] + cv[i]) * VX_OUT_MW);
                hr[p].assign(orr.begin() + ro[i] * nt, orr.begin() + (ro[i] + cr[i]) * nt);
            }
        }
        stats.slab = cap;
        if (over.empty()) break;
        // repeat only the overflowed polytopes with a four times larger slab, while one polytope's slab fits the budget
        const long long next = cap * 4;
        if (next > max_slab || vx_slab_bytes<NT>(next) > budget) break;
        stats.repeats += (int64_t)over.size();
        pending.swap(over);
        cap = next;
    }
    return s.finish();
}

extern "C" int mpc_region_vertices(int32_t device, int32_t n_t, int64_t n_poly, const int64_t *row_off, const double *ef_rows, double tol,
                                   int64_t slab, int64_t max_slab, int64_t budget, int64_t *v_cap, int64_t *r_cap, int32_t *status,
                                   int64_t *n_vert, int64_t *n_ray, double *vertices, uint64_t *incidence, double *rays,
                                   mpc_vertex_stats *stats) {
    const char *who = "mpc_region_vertices";
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_t < 1 || n_t > 16) return bad(who, "n_theta must lie in 1..16");
    if (n_poly < 0 || n_poly > (1ll << 31) - 1) return bad(who, "n_poly must lie in 0..2^31-1");
    if (!row_off || !v_cap || !r_cap) return bad(who, "missing row_off, v_cap or r_cap");
    if (row_off[0] != 0) return bad(who, "row_off[0] must be 0");
    for (int64_t p = 0; p < n_poly; ++p) {
        const int64_t r = row_off[p + 1] - row_off[p];
        if (r < 0) return bad(who, "row_off decreases");
        if (r > VX_MAX_ROWS) return bad(who, "polytope " + std::to_string(p) + " has " + std::to_string(r) + " rows, more than " + std::to_string(VX_MAX_ROWS));
    }
    const long long rows = row_off[n_poly];
    if (rows && !ef_rows) return bad(who, "missing ef_rows");
    for (long long i = 0; i < rows * (n_t + 1); ++i)
        if (!std::isfinite(ef_rows[i])) return bad(who, "the rows must be finite (row " + std::to_string(i / (n_t + 1)) + ")");
    if (!std::isfinite(tol) || tol < 0.0) return bad(who, "tol must be finite and >= 0");
    const long long slab0 = slab > 0 ? slab : VX_DEFAULT_SLAB, smax = max_slab > 0 ? max_slab : VX_MAX_SLAB;
    if (slab0 < 18 || slab0 > smax || smax > VX_MAX_SLAB) return bad(who, "need 18 <= slab <= max_slab <= 2^24 generators");
    const double cap_bytes = budget > 0 ? (double)budget : (double)VX_DEFAULT_BUDGET;
    const double per = with_width(n_t, [&](auto W) { return vx_slab_bytes<decltype(W)::value>(slab0); });
    if (per > cap_bytes)
        return bad(who, "the budget of " + std::to_string((long long)cap_bytes) + " device bytes is too small for one polytope's slab (" +
                   std::to_string((long long)per) + " bytes)");
    if (n_poly > 0 && (!status || !n_vert || !n_ray)) return bad(who, "missing status, n_vert or n_ray");
    if (n_poly == 0) { *v_cap = 0; *r_cap = 0; return MPC_OK; }
    if (int rc = select_device(who, device)) return rc;
    std::vector<int32_t> st(n_poly, VX_OVERFLOW);
    std::vector<int64_t> nv(n_poly, 0), nr(n_poly, 0);
    std::vector<std::vector<double>> hv(n_poly), hr(n_poly);
    std::vector<std::vector<uint64_t>> hz(n_poly);
    mpc_vertex_stats s{};
    if (int rc = with_width(n_t, [&](auto W) {
            return vx_run<decltype(W)::value>(who, n_t, n_poly, row_off, ef_rows, tol, slab0, smax, cap_bytes, st, nv, nr, hv, hz, hr, s);
        })) return rc;
    long long tv = 0, tr = 0;
    for (int64_t p = 0; p < n_poly; ++p) {
        status[p] = st[p]; n_vert[p] = nv[p]; n_ray[p] = nr[p];
        if (st[p] == VX_OVERFLOW) s.overflow += 1;
        tv += nv[p]; tr += nr[p];
    }
    if (stats) *stats = s;
    const bool fits = tv <= *v_cap && tr <= *r_cap;
    *v_cap = tv; *r_cap = tr;
    if (!fits) return fail(nullptr, MPC_ERR_CAPACITY, std::string(who) + ": the outputs need " + std::to_string(tv) + " vertices and " +
                                                            std::to_string(tr) + " rays (returned in v_cap, r_cap)");
    if ((tv && (!vertices || !incidence)) || (tr && !rays)) return bad(who, "missing vertices, incidence or rays");
    long long pv = 0, pr = 0;
    for (int64_t p = 0; p < n_poly; ++p) {
        if (nv[p]) {
            std::memcpy(vertices + pv * n_t, hv[p].data(), hv[p].size() * 8);
            std::memcpy(incidence + pv * VX_OUT_MW, hz[p].data(), hz[p].size() * 8);
        }
        if (nr[p]) std::memcpy(rays + pr * n_t, hr[p].data(), hr[p].size() * 8);
        pv += nv[p]; pr += nr[p];
    }
    return MPC_OK;
}

// ---- volumes and centroids of a batch of polytopes from their vertex lists (volume.hpp) ---------------------------------
constexpr long long VOL_DEFAULT_BUDGET = 4ll << 30, VOL_MAX_CHUNK_ITEMS = 1ll << 26;
constexpr long long VOL_LDS_WORDS[3] = {512, 2048, 5120};   // classes of stack + Ct words per wave: 4, 16, 40 KB of LDS; beyond: Ct in global memory

// device bytes one polytope of m rows and nv vertices adds to a chunk: its Ct (m words per 64 vertices), its counter and its chunk entries;
// m2_entries: the entries of a second-moment slot (0: the volume pass), one slot per row
static long long vol_poly_bytes(long long m, long long nv, long long m2_entries) {
    return m * ((nv + 63) / 64) * 8 + 8 + 4 + 8 + m * 8 + m * m2_entries * 8;
}

// second_moment: [n_poly][nt][nt], or nullptr for the volume pass (the M2 = false kernels)
template <int NT>
static int vol_run(const char *who, int nt, int64_t n_poly, const int64_t *row_off, const int64_t *vert_off, const double *vertices,
                   const uint64_t *incidence, const std::vector<int32_t> &todo, long long max_simplices, long long budget, double *volume,
                   double *centroid, int64_t *n_simplices, int32_t *status, double *second_moment, mpc_volume_stats &stats) {
    OneShot s(who, nullptr, true);
    const long long rows = row_off[n_poly], nv_all = vert_off[n_poly];
    const bool m2 = second_moment != nullptr;
    const long long ne = m2 ? (long long)nt * (nt + 1) / 2 : 0;
    DevBuf &d_roff = s.upload(row_off, (size_t)(n_poly + 1) * 8), &d_voff = s.upload(vert_off, (size_t)(n_poly + 1) * 8);
    DevBuf &d_vert = s.upload(vertices, (size_t)nv_all * nt * 8), &d_inc = s.upload(incidence, (size_t)nv_all * 4 * 8);
    DevBuf &d_svol = s.buf((size_t)rows * 8), &d_smom = s.buf((size_t)rows * nt * 8), &d_scnt = s.buf((size_t)rows * 8), &d_sst = s.buf((size_t)rows * 4);
    DevBuf &d_vol = s.buf((size_t)n_poly * 8), &d_cen = s.buf((size_t)n_poly * nt * 8), &d_ns = s.buf((size_t)n_poly * 8), &d_st = s.buf((size_t)n_poly * 4);
    DevBuf &d_chunk = s.buf(), &d_ctoff = s.buf(), &d_ct = s.buf(), &d_count = s.buf();
    DevBuf &d_sm2 = s.buf((size_t)rows * ne * 8), &d_m2 = s.buf((size_t)(m2 ? n_poly * nt * nt : 0) * 8);
    DevBuf *d_iq[4], *d_ir[4];
    for (int c = 0; c < 4; ++c) { d_iq[c] = &s.buf(); d_ir[c] = &s.buf(); }
    for (size_t start = 0; start < todo.size();) {
        // a chunk: as many polytopes as the budget holds
        std::vector<int32_t> chunk;
        std::vector<long long> ct_off;
        std::vector<int32_t> iq[4], ir[4];
        long long lds_words[4] = {0, 0, 0, 0};
        long long bytes = 0, words = 0, items = 0;
        while (start < todo.size()) {
            const int32_t p = todo[start];
            const long long m = row_off[p + 1] - row_off[p], nv = vert_off[p + 1] - vert_off[p], W = (nv + 63) / 64;
            if (!chunk.empty() && (bytes + vol_poly_bytes(m, nv, ne) > budget || items + m > VOL_MAX_CHUNK_ITEMS)) break;
            const long long stack = (long long)nt * W, need = stack + m * W;
            const int cls = need <= VOL_LDS_WORDS[0] ? 0 : need <= VOL_LDS_WORDS[1] ? 1 : need <= VOL_LDS_WORDS[2] ? 2 : 3;
            lds_words[cls] = std::max(lds_words[cls], cls < 3 ? need : stack);
            for (long long r = 0; r < m; ++r) { iq[cls].push_back((int32_t)chunk.size()); ir[cls].push_back((int32_t)r); }
            chunk.push_back(p);
            ct_off.push_back(words);
            bytes += vol_poly_bytes(m, nv, ne); words += m * W; items += m;
            ++start;
        }
        const long long nq = (long long)chunk.size();
        s.upload(d_chunk, chunk.data(), (size_t)nq * 4);
        s.upload(d_ctoff, ct_off.data(), (size_t)nq * 8);
        s.ensure(d_ct, std::max<size_t>(8, (size_t)words * 8));
        s.ensure(d_count, (size_t)nq * 8);
        s.fill(d_count, 0, (size_t)nq * 8);
        for (int c = 0; c < 4; ++c) { s.upload(*d_iq[c], iq[c].data(), iq[c].size() * 4); s.upload(*d_ir[c], ir[c].data(), ir[c].size() * 4); }
        int launches = 0;
        s.launch_timed([&] {
            hipLaunchKernelGGL(k_volume_rowsets, dim3((unsigned)nq), dim3(VOL_ROWSET_BLOCK), 0, nullptr, d_chunk.as<int32_t>(), d_roff.as<long long>(),
                               d_voff.as<long long>(), d_inc.as<unsigned long long>(), d_ctoff.as<long long>(), d_ct.as<unsigned long long>());
            ++launches;
            for (int c = 0; c < 4; ++c) {
                if (iq[c].empty()) continue;
                VolArgs a{};
                a.nt = nt; a.c_in_lds = c < 3; a.n_items = (long long)iq[c].size(); a.item_q = d_iq[c]->as<int32_t>(); a.item_row = d_ir[c]->as<int32_t>();
                a.chunk_poly = d_chunk.as<int32_t>(); a.row_off = d_roff.as<long long>(); a.vert_off = d_voff.as<long long>(); a.vert = d_vert.as<double>();
                a.ct = d_ct.as<unsigned long long>(); a.ct_off = d_ctoff.as<long long>(); a.max_simplices = max_simplices;
                a.poly_count = d_count.as<unsigned long long>(); a.slot_vol = d_svol.as<double>(); a.slot_mom = d_smom.as<double>();
                a.slot_cnt = d_scnt.as<long long>(); a.slot_st = d_sst.as<int32_t>(); a.slot_m2 = d_sm2.as<double>();
                const dim3 grid((unsigned)iq[c].size());
                if (m2) hipLaunchKernelGGL((k_volume_walk<NT, true>), grid, dim3(64), (size_t)lds_words[c] * 8, nullptr, a);
                else hipLaunchKernelGGL((k_volume_walk<NT, false>), grid, dim3(64), (size_t)lds_words[c] * 8, nullptr, a);
                ++launches;
            }
            const dim3 rgrid((unsigned)((nq + 63) / 64), m2 ? (unsigned)ne : 1u);
            auto reduce = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, rgrid, dim3(64), 0, nullptr, nt, nq, d_chunk.as<int32_t>(), d_roff.as<long long>(), max_simplices,
                                   d_svol.as<double>(), d_smom.as<double>(), d_scnt.as<long long>(), d_sst.as<int32_t>(), d_sm2.as<double>(),
                                   d_vol.as<double>(), d_cen.as<double>(), d_ns.as<long long>(), d_st.as<int32_t>(), d_m2.as<double>());
            };
            if (m2) reduce(k_volume_reduce<true>); else reduce(k_volume_reduce<false>);
            ++launches;
        });
        s.sync();
        s.synced = false;
        float ms = 0.0f;
        s.elapsed(&ms);
        if (!s.ok()) return s.finish();
        stats.ms += ms;
        stats.launches += launches;
    }
    std::vector<double> hv((size_t)n_poly), hc((size_t)n_poly * nt);
    std::vector<long long> hn((size_t)n_poly);
    std::vector<int32_t> hs((size_t)n_poly);
    s.download(hv.data(), d_vol, hv.size() * 8);
    s.download(hc.data(), d_cen, hc.size() * 8);
    s.download(hn.data(), d_ns, hn.size() * 8);
    s.download(hs.data(), d_st, hs.size() * 4);
    std::vector<double> hm((size_t)(m2 ? n_poly * nt * nt : 0));
    if (m2) s.download(hm.data(), d_m2, hm.size() * 8);
    if (!s.ok()) return s.finish();
    for (int32_t p : todo) {
        volume[p] = hv[(size_t)p]; n_simplices[p] = hn[(size_t)p]; status[p] = hs[(size_t)p];
        std::memcpy(centroid + (size_t)p * nt, hc.data() + (size_t)p * nt, (size_t)nt * 8);
        if (m2) std::memcpy(second_moment + (size_t)p * nt * nt, hm.data() + (size_t)p * nt * nt, (size_t)nt * nt * 8);
    }
    return s.finish();
}

// mpc_region_volumes (want_m2 = false) and mpc_region_moments: the checks, what needs no walk, the walk and the statistics
static int vol_entry(const char *who, bool want_m2, int32_t device, int32_t n_t, int64_t n_poly, const int64_t *row_off, const double *ef_rows,
                     const int64_t *vert_off, const double *vertices, const uint64_t *incidence, const int32_t *vx_status, double tol,
                     int64_t max_simplices, int64_t budget, double *volume, double *centroid, int64_t *n_simplices, int32_t *status,
                     double *second_moment, mpc_volume_stats *stats) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_t < 1 || n_t > 16) return bad(who, "n_theta must lie in 1..16");
    if (n_poly < 0 || n_poly > (1ll << 31) - 1) return bad(who, "n_poly must lie in 0..2^31-1");
    if (!row_off || !vert_off) return bad(who, "missing row_off or vert_off");
    if (row_off[0] != 0 || vert_off[0] != 0) return bad(who, "row_off[0] and vert_off[0] must be 0");
    if (max_simplices < 1) return bad(who, "max_simplices must be >= 1");
    if (!std::isfinite(tol) || tol < 0.0) return bad(who, "tol must be finite and >= 0");
    const long long limit = budget > 0 ? budget : VOL_DEFAULT_BUDGET;
    const long long ne = want_m2 ? (long long)n_t * (n_t + 1) / 2 : 0;
    for (int64_t p = 0; p < n_poly; ++p) {
        const int64_t r = row_off[p + 1] - row_off[p], v = vert_off[p + 1] - vert_off[p];
        if (r < 0 || v < 0) return bad(who, "row_off or vert_off decreases");
        if (r > VOL_MAX_ROWS) return bad(who, "polytope " + std::to_string(p) + " has " + std::to_string(r) + " rows, more than " + std::to_string(VOL_MAX_ROWS));
        if (v <= VOL_MAX_VERTS && vol_poly_bytes(r, v, ne) > limit)
            return bad(who, "the budget of " + std::to_string(limit) + " device bytes is too small for polytope " + std::to_string(p) + " (" +
                       std::to_string(vol_poly_bytes(r, v, ne)) + " bytes)");
    }
    const long long rows = row_off[n_poly], nv_all = vert_off[n_poly];
    if ((rows && !ef_rows) || (nv_all && (!vertices || !incidence))) return bad(who, "missing ef_rows, vertices or incidence");
    for (long long i = 0; i < rows * (n_t + 1); ++i)
        if (!std::isfinite(ef_rows[i])) return bad(who, "the rows must be finite (row " + std::to_string(i / (n_t + 1)) + ")");
    for (long long i = 0; i < nv_all * n_t; ++i)
        if (!std::isfinite(vertices[i])) return bad(who, "the vertices must be finite (vertex " + std::to_string(i / n_t) + ")");
    if (n_poly == 0) return MPC_OK;
    if (!vx_status || !volume || !centroid || !n_simplices || !status || (want_m2 && !second_moment)) return bad(who, "missing vx_status or an output array");
    const double nan = std::nan(""), inf = HUGE_VAL;
    std::vector<int32_t> todo;
    for (int64_t p = 0; p < n_poly; ++p) {
        const int32_t vs = vx_status[p];
        if (vs < VOL_OK || vs > VOL_OVERFLOW) return bad(who, "vx_status[" + std::to_string(p) + "] is not a status of mpc_region_vertices");
        const int64_t v = vert_off[p + 1] - vert_off[p];
        // what needs no walk: the statuses of the vertex pass, and a vertex list too long for the stack of a wave
        status[p] = vs != VOL_OK ? vs : v > VOL_MAX_VERTS ? VOL_TOO_LARGE : v < 1 || row_off[p + 1] == row_off[p] ? VOL_INCONSISTENT : VOL_OK;
        n_simplices[p] = 0;
        volume[p] = vs == VOL_EMPTY ? 0.0 : (vs == VOL_UNBOUNDED || vs == VOL_NOT_POINTED) ? inf : nan;
        for (int c = 0; c < n_t; ++c) centroid[p * n_t + c] = nan;
        if (want_m2) for (int c = 0; c < n_t * n_t; ++c) second_moment[p * n_t * n_t + c] = vs == VOL_EMPTY ? 0.0 : nan;
        if (status[p] == VOL_OK && vs == VOL_OK) todo.push_back((int32_t)p);
    }
    mpc_volume_stats st{};
    if (!todo.empty()) {
        if (int rc = select_device(who, device)) return rc;
        if (int rc = with_width(n_t, [&](auto W) {
                return vol_run<decltype(W)::value>(who, n_t, n_poly, row_off, vert_off, vertices, incidence, todo, max_simplices, limit, volume, centroid,
                                                   n_simplices, status, want_m2 ? second_moment : nullptr, st);
            })) return rc;
    }
    for (int64_t p = 0; p < n_poly; ++p) {
        st.status_counts[status[p]] += 1;
        st.simplices += n_simplices[p];
        st.max_simplices = std::max<int64_t>(st.max_simplices, n_simplices[p]);
    }
    if (stats) *stats = st;
    return MPC_OK;
}

extern "C" int mpc_region_volumes(int32_t device, int32_t n_t, int64_t n_poly, const int64_t *row_off, const double *ef_rows, const int64_t *vert_off,
                                  const double *vertices, const uint64_t *incidence, const int32_t *vx_status, double tol, int64_t max_simplices,
                                  int64_t budget, double *volume, double *centroid, int64_t *n_simplices, int32_t *status, mpc_volume_stats *stats) {
    return vol_entry("mpc_region_volumes", false, device, n_t, n_poly, row_off, ef_rows, vert_off, vertices, incidence, vx_status, tol, max_simplices,
                     budget, volume, centroid, n_simplices, status, nullptr, stats);
}

// second moments with the volumes and centroids (volume.hpp M2 = true)
extern "C" int mpc_region_moments(int32_t device, int32_t n_t, int64_t n_poly, const int64_t *row_off, const double *ef_rows, const int64_t *vert_off,
                                  const double *vertices, const uint64_t *incidence, const int32_t *vx_status, double tol, int64_t max_simplices,
                                  int64_t budget, double *volume, double *centroid, int64_t *n_simplices, int32_t *status, double *second_moment,
                                  mpc_volume_stats *stats) {
    return vol_entry("mpc_region_moments", true, device, n_t, n_poly, row_off, ef_rows, vert_off, vertices, incidence, vx_status, tol, max_simplices,
                     budget, volume, centroid, n_simplices, status, second_moment, stats);
}

// ---- the family of wavefront-per-item LP calls: region merging, overlap removal, transition graph, exit sets, row reduction, backward exits,
// projection (merge.hpp, overlap.hpp, transition.hpp, exit_sets.hpp, reduce.hpp, invariant.hpp, project.hpp)  Every call checks its arguments in one order
// (regions, pieces, tol, the item count, the dense arrays, the empty batch, missing arrays, the index arrays, the rest), uploads,
// launches one wavefront per item over unit rows [o | n] in LDS, and downloads the results and its counters.  What the calls share is
// here once: the checkers return the refusal, family_launch and family_close are the two ends of the device part.
static void family_open(int64_t *stats, int n_stats, float *ms) {
    if (stats) for (int i = 0; i < n_stats; ++i) stats[i] = 0;
    if (ms) *ms = 0.0f;
}

static int check_tol(const char *who, double tol) { return std::isfinite(tol) && tol >= 0.0 ? (int)MPC_OK : bad(who, "tol must be finite and >= 0"); }

// name: "n_pairs" or "n_items"
static int check_count(const char *who, const char *name, int64_t n) {
    return n >= 0 && n <= 0x7fffffffll ? (int)MPC_OK : bad(who, std::string(name) + " must lie in 0..2^31 - 1");
}

static int check_finite(const char *who, const char *name, const double *v, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return bad(who, std::string(name) + " must be finite");
    return MPC_OK;
}

// the rows k of [n][n_t + 1] with only[k] != 0 (only == nullptr: all of them) are finite with unit normals
static int check_unit_rows(const char *who, const char *what, int32_t n_t, int64_t n, const double *rows, const int32_t *only) {
    for (int64_t k = 0; k < n; ++k) {
        if (only && !only[k]) continue;
        const double *row = rows + k * (n_t + 1);
        double nn = 0.0;
        bool finite = std::isfinite(row[0]);
        for (int t = 0; t < n_t; ++t) { nn += row[1 + t] * row[1 + t]; finite = finite && std::isfinite(row[1 + t]); }
        if (!finite || !(std::fabs(std::sqrt(nn) - 1.0) <= 1e-6)) return bad(who, std::string(what) + " must be finite with unit normals");
    }
    return MPC_OK;
}

// One index array of a call's items: item k names polytope v[k] of 0..n-1; off != nullptr: its rows off[v + 1] - off[v] lie in LDS.
struct IndexArray { const int32_t *v; int64_t n; const int64_t *off; };
// Refuses with ``why`` an item with an index out of range or, with ``distinct``, the same index in the first two arrays; raises *rows
// to the largest sum over an item of the rows in LDS plus ``extra``.
static int check_indices(const char *who, const char *why, int64_t n_items, std::initializer_list<IndexArray> arrays, bool distinct, int extra,
                         int *rows) {
    for (int64_t k = 0; k < n_items; ++k) {
        int64_t sum = extra;
        for (const IndexArray &a : arrays) {
            const int64_t i = a.v[k];
            if (i < 0 || i >= a.n) return bad(who, why);
            if (a.off) sum += a.off[i + 1] - a.off[i];
        }
        if (distinct && arrays.begin()[0].v[k] == arrays.begin()[1].v[k]) return bad(who, why);
        *rows = std::max<int>(*rows, (int)sum);
    }
    return MPC_OK;
}

// a zeroed buffer of n counters
static DevBuf &family_counters(OneShot &s, int n) {
    DevBuf &d_cnt = s.buf((size_t)n * 8);
    s.fill(d_cnt, 0, (size_t)n * 8);
    return d_cnt;
}

// kernel<<<n wavefronts, 64, lds>>>(args...) between the two events of s
template <class K, class... A> static void family_launch(OneShot &s, K kernel, int64_t n, size_t lds, A... args) {
    if (s.ok() && lds > 48 * 1024)
        s.chk(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    s.launch_timed([&] { hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(64), lds, nullptr, args...); });
}

// the n counters to stats, the device time to ms, and the call's code
static int family_close(OneShot &s, const DevBuf &d_cnt, int n, int64_t *stats, float *ms) {
    unsigned long long cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    s.download(cnt, d_cnt, (size_t)n * 8);
    if (stats) for (int i = 0; i < n; ++i) stats[i] = (int64_t)cnt[i];
    s.elapsed(ms);
    return s.finish();
}

// ---- merging regions with equal laws (merge.hpp) ---------------------------------------------------------------------
// max_rows: MG_MAX_ROWS for every call but mpc_reduce_rows (RD_MAX_ROWS)
static int merge_check(const char *who, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, int *m_max,
                       int max_rows = MG_MAX_ROWS) {
    if (n_t < 1 || n_t > TR_MAX_NT) return bad(who, "n_t must lie in 1..16");
    if (n_regions < 0 || (n_regions > 0 && !row_off)) return bad(who, "bad region count or missing row_off");
    if (n_regions > 0x7fffffffll) return bad(who, "too many regions for one launch");
    if (n_regions > 0 && row_off[0] != 0) return bad(who, "row_off[0] must be 0");
    *m_max = 1;
    for (int64_t r = 0; r < n_regions; ++r) {
        const int64_t k = row_off[r + 1] - row_off[r];
        if (k < 1 || k > max_rows) return bad(who, "every region needs 1.." + std::to_string(max_rows) + " rows");
        *m_max = std::max<int>(*m_max, (int)k);
    }
    const int64_t rows = n_regions > 0 ? row_off[n_regions] : 0;
    if (rows > 0 && !ef_rows) return bad(who, "missing ef_rows");
    return check_unit_rows(who, "rows", n_t, rows, ef_rows, nullptr);
}

extern "C" int mpc_merge_regions(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, double *xs,
                                 double *box, int32_t *status, int64_t *stats, float *ms) {
    const char *who = "mpc_merge_regions";
    family_open(stats, 3, ms);
    int m_max = 1;
    if (int rc = merge_check(who, n_t, n_regions, row_off, ef_rows, &m_max)) return rc;
    if (n_regions == 0) return MPC_OK;
    if (!xs || !box || !status) return bad(who, "missing output array");
    if (int rc = select_device(nullptr, device)) return rc;
    const size_t nr = (size_t)n_regions;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_regions, row_off, ef_rows, n_t + 1);
    DevBuf &d_xs = s.buf(nr * n_t * 8), &d_box = s.buf(nr * 2 * n_t * 8), &d_st = s.buf(nr * 4), &d_cnt = family_counters(s, 3);
    family_launch(s, k_merge_regions, n_regions, tr_lds_bytes(m_max, n_t), (int)n_t, m_max, (long long)n_regions, d.off.as<long long>(),
                  d.ef.as<double>(), d_xs.as<double>(), d_box.as<double>(), d_st.as<int32_t>(), d_cnt.as<unsigned long long>());
    s.download(xs, d_xs, nr * n_t * 8);
    s.download(box, d_box, nr * 2 * n_t * 8);
    s.download(status, d_st, nr * 4);
    return family_close(s, d_cnt, 3, stats, ms);
}

extern "C" int mpc_merge_pairs(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *xs,
                               const double *box, int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, double tol, uint64_t *env_a,
                               uint64_t *env_b, int32_t *verdict, double *t_max, int64_t *stats, float *ms) {
    const char *who = "mpc_merge_pairs";
    family_open(stats, 7, ms);
    int m_max = 1;
    if (int rc = merge_check(who, n_t, n_regions, row_off, ef_rows, &m_max)) return rc;
    if (int rc = check_tol(who, tol)) return rc;
    if (int rc = check_count(who, "n_pairs", n_pairs)) return rc;
    if (n_pairs == 0) return MPC_OK;
    if (!xs || !box || !pair_a || !pair_b || !env_a || !env_b || !verdict || !t_max) return bad(who, "missing array");
    int pair_rows = 2;
    if (int rc = check_indices(who, "a pair names a region out of range, or the same region twice", n_pairs,
                               {{pair_a, n_regions, row_off}, {pair_b, n_regions, row_off}}, true, 2, &pair_rows)) return rc;
    if (int rc = check_finite(who, "xs", xs, n_regions * n_t)) return rc;
    if (int rc = select_device(nullptr, device)) return rc;
    const int lds_rows = std::max(pair_rows, m_max);
    const size_t lds = tr_lds_bytes(lds_rows, n_t);   // 514 rows at n_t = 16: 79,132 bytes (the static s_env adds 64)
    const size_t np = (size_t)n_pairs, words = np * MG_WORDS * 8;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_regions, row_off, ef_rows, n_t + 1);
    DevBuf &d_xs = s.upload(xs, (size_t)n_regions * n_t * 8), &d_box = s.upload(box, (size_t)n_regions * 2 * n_t * 8);
    DevBuf &d_pa = s.upload(pair_a, np * 4), &d_pb = s.upload(pair_b, np * 4);
    DevBuf &d_ea = s.buf(words), &d_eb = s.buf(words), &d_v = s.buf(np * 4), &d_t = s.buf(np * 8), &d_cnt = family_counters(s, 7);
    MergePairArgs a{};
    a.nt = n_t; a.m_max = lds_rows; a.n_pairs = n_pairs;
    a.row_off = d.off.as<long long>(); a.ef = d.ef.as<double>(); a.xs = d_xs.as<double>(); a.box = d_box.as<double>();
    a.pair_a = d_pa.as<int32_t>(); a.pair_b = d_pb.as<int32_t>(); a.tol = tol;
    a.env_a = d_ea.as<unsigned long long>(); a.env_b = d_eb.as<unsigned long long>(); a.verdict = d_v.as<int32_t>(); a.t_max = d_t.as<double>();
    a.counters = d_cnt.as<unsigned long long>();
    family_launch(s, k_merge_pairs, n_pairs, lds, a);
    s.download(env_a, d_ea, words);
    s.download(env_b, d_eb, words);
    s.download(verdict, d_v, np * 4);
    s.download(t_max, d_t, np * 8);
    return family_close(s, d_cnt, 7, stats, ms);
}

// ---- overlap removal by lowest objective (overlap.hpp) --------------------------------------------------------------
// has_cut [n] and the cut rows [n][n_t + 1] it selects: finite with unit normals
static int overlap_check_cuts(const char *who, int32_t n_t, int64_t n, const int32_t *has_cut, const double *cut_rows) {
    if (!has_cut) return bad(who, "missing has_cut");
    if (cut_rows) return check_unit_rows(who, "cut rows", n_t, n, cut_rows, has_cut);
    return std::any_of(has_cut, has_cut + n, [](int32_t h) { return h != 0; }) ? bad(who, "missing cut_rows") : (int)MPC_OK;
}

extern "C" int mpc_overlap_pairs(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *xs,
                                 int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, const int32_t *has_cut, const double *cut_rows,
                                 double tol, double *radius, double *d_min, double *d_max, int32_t *flag, int64_t *stats, float *ms) {
    const char *who = "mpc_overlap_pairs";
    family_open(stats, 4, ms);
    int m_max = 1;
    if (int rc = merge_check(who, n_t, n_regions, row_off, ef_rows, &m_max)) return rc;
    if (int rc = check_tol(who, tol)) return rc;
    if (int rc = check_count(who, "n_pairs", n_pairs)) return rc;
    if (n_pairs == 0) return MPC_OK;
    if (!xs || !pair_a || !pair_b || !radius || !d_min || !d_max || !flag) return bad(who, "missing array");
    int pair_rows = 2;
    if (int rc = check_indices(who, "a pair names a region out of range, or the same region twice", n_pairs,
                               {{pair_a, n_regions, row_off}, {pair_b, n_regions, row_off}}, true, 0, &pair_rows)) return rc;
    if (int rc = overlap_check_cuts(who, n_t, n_pairs, has_cut, cut_rows)) return rc;
    if (int rc = check_finite(who, "xs", xs, n_regions * n_t)) return rc;
    if (int rc = select_device(nullptr, device)) return rc;
    const size_t lds = tr_lds_bytes(pair_rows, n_t);   // 512 rows at n_t = 16: 78,840 bytes
    const size_t np = (size_t)n_pairs;
    const double zero_row = 0.0;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_regions, row_off, ef_rows, n_t + 1);
    DevBuf &d_xs = s.upload(xs, (size_t)n_regions * n_t * 8), &d_pa = s.upload(pair_a, np * 4), &d_pb = s.upload(pair_b, np * 4);
    DevBuf &d_hc = s.upload(has_cut, np * 4), &d_cut = cut_rows ? s.upload(cut_rows, np * (n_t + 1) * 8) : s.upload(&zero_row, 8);
    DevBuf &d_r = s.buf(np * 8), &d_lo = s.buf(np * 8), &d_hi = s.buf(np * 8), &d_f = s.buf(np * 4), &d_cnt = family_counters(s, 4);
    OverlapPairArgs a{};
    a.nt = n_t; a.m_max = pair_rows; a.n_pairs = n_pairs;
    a.row_off = d.off.as<long long>(); a.ef = d.ef.as<double>(); a.xs = d_xs.as<double>();
    a.pair_a = d_pa.as<int32_t>(); a.pair_b = d_pb.as<int32_t>(); a.has_cut = d_hc.as<int32_t>(); a.cut = d_cut.as<double>(); a.tol = tol;
    a.radius = d_r.as<double>(); a.d_min = d_lo.as<double>(); a.d_max = d_hi.as<double>(); a.flag = d_f.as<int32_t>();
    a.counters = d_cnt.as<unsigned long long>();
    family_launch(s, k_overlap_pairs, n_pairs, lds, a);
    s.download(radius, d_r, np * 8);
    s.download(d_min, d_lo, np * 8);
    s.download(d_max, d_hi, np * 8);
    s.download(flag, d_f, np * 4);
    return family_close(s, d_cnt, 4, stats, ms);
}

extern "C" int mpc_overlap_split(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, int64_t n_pieces,
                                 const int64_t *piece_off, const double *piece_rows, int64_t n_items, const int32_t *item_piece,
                                 const int32_t *item_cutter, const int32_t *has_cut, const double *cut_rows, const double *start, double tol,
                                 int32_t *flag, uint64_t *mask, int64_t *stats, float *ms) {
    const char *who = "mpc_overlap_split";
    family_open(stats, 5, ms);
    int m_reg = 1, m_piece = 1;
    if (int rc = merge_check(who, n_t, n_regions, row_off, ef_rows, &m_reg)) return rc;
    if (int rc = merge_check("mpc_overlap_split (pieces)", n_t, n_pieces, piece_off, piece_rows, &m_piece)) return rc;
    if (int rc = check_tol(who, tol)) return rc;
    if (int rc = check_count(who, "n_items", n_items)) return rc;
    if (n_items == 0) return MPC_OK;
    if (!item_piece || !item_cutter || !flag || !mask) return bad(who, "missing array");
    int item_rows = 4;
    if (int rc = check_indices(who, "an item names a piece or a cutter out of range", n_items,
                               {{item_piece, n_pieces, piece_off}, {item_cutter, n_regions, row_off}}, false, 2, &item_rows)) return rc;
    if (int rc = overlap_check_cuts(who, n_t, n_items, has_cut, cut_rows)) return rc;
    if (start)
        if (int rc = check_finite(who, "start", start, n_items * n_t)) return rc;
    if (int rc = select_device(nullptr, device)) return rc;
    const size_t lds = tr_lds_bytes(item_rows, n_t);   // 514 rows at n_t = 16: 79,132 bytes (the static s_mask adds 32)
    const size_t ni = (size_t)n_items, words = ni * OV_WORDS * 8;
    const double zero_row = 0.0;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_regions, row_off, ef_rows, n_t + 1);
    const RegionsOnDevice pc = upload_regions(s, n_pieces, piece_off, piece_rows, n_t + 1);
    DevBuf &d_ip = s.upload(item_piece, ni * 4), &d_ic = s.upload(item_cutter, ni * 4), &d_hc = s.upload(has_cut, ni * 4);
    DevBuf &d_cut = cut_rows ? s.upload(cut_rows, ni * (n_t + 1) * 8) : s.upload(&zero_row, 8);
    DevBuf *d_start = start ? &s.upload(start, ni * n_t * 8) : nullptr;
    DevBuf &d_f = s.buf(ni * 4), &d_m = s.buf(words), &d_cnt = family_counters(s, 5);
    OverlapSplitArgs a{};
    a.nt = n_t; a.m_max = item_rows; a.n_items = n_items;
    a.row_off = d.off.as<long long>(); a.ef = d.ef.as<double>(); a.piece_off = pc.off.as<long long>(); a.piece_ef = pc.ef.as<double>();
    a.item_piece = d_ip.as<int32_t>(); a.item_cutter = d_ic.as<int32_t>(); a.has_cut = d_hc.as<int32_t>(); a.cut = d_cut.as<double>();
    a.start = d_start ? d_start->as<double>() : nullptr; a.tol = tol;
    a.flag = d_f.as<int32_t>(); a.mask = d_m.as<unsigned long long>(); a.counters = d_cnt.as<unsigned long long>();
    family_launch(s, k_overlap_split, n_items, lds, a);
    s.download(flag, d_f, ni * 4);
    s.download(mask, d_m, words);
    return family_close(s, d_cnt, 5, stats, ms);
}

// ---- the largest law gap of region pairs (compare.hpp) -----------------------------------------------------------------
extern "C" int mpc_law_gap_pairs(int32_t device, int32_t n_t, int32_t n_out, int64_t n_regions, const int64_t *row_off, const double *ef_rows,
                                 const double *laws, const double *xs, int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, double tol,
                                 double *radius, double *gap, int32_t *gap_row, double *witness, double *range, int32_t *flag, int64_t *stats,
                                 float *ms) {
    const char *who = "mpc_law_gap_pairs";
    family_open(stats, 6, ms);
    int m_max = 1;
    if (int rc = merge_check(who, n_t, n_regions, row_off, ef_rows, &m_max)) return rc;
    if (n_out < 1 || n_out > LG_MAX_OUT) return bad(who, "n_out must lie in 1..256");
    if (int rc = check_tol(who, tol)) return rc;
    if (int rc = check_count(who, "n_pairs", n_pairs)) return rc;
    if (n_regions > 0 && (!laws || !xs)) return bad(who, "missing array (laws or xs)");
    if (int rc = check_finite(who, "laws", laws, n_regions * n_out * (n_t + 1))) return rc;
    if (int rc = check_finite(who, "xs", xs, n_regions * n_t)) return rc;
    if (n_pairs == 0) return MPC_OK;
    if (!pair_a || !pair_b || !radius || !gap || !gap_row || !witness || !flag) return bad(who, "missing array");
    int pair_rows = 2;     // i == j is legal: a region against itself, gap 0
    if (int rc = check_indices(who, "a pair names a region out of range", n_pairs, {{pair_a, n_regions, row_off}, {pair_b, n_regions, row_off}}, false,
                               0, &pair_rows)) return rc;
    if (int rc = select_device(nullptr, device)) return rc;
    const size_t lds = tr_lds_bytes(pair_rows, n_t);   // 512 rows at n_t = 16: 78,840 bytes (the static arrays add 408)
    const size_t np = (size_t)n_pairs, nr = (size_t)n_regions;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_regions, row_off, ef_rows, n_t + 1);
    DevBuf &d_laws = s.upload(laws, nr * n_out * (n_t + 1) * 8), &d_xs = s.upload(xs, nr * n_t * 8);
    DevBuf &d_pa = s.upload(pair_a, np * 4), &d_pb = s.upload(pair_b, np * 4);
    DevBuf &d_r = s.buf(np * 8), &d_g = s.buf(np * 8), &d_row = s.buf(np * 4), &d_w = s.buf(np * n_t * 8), &d_f = s.buf(np * 4);
    DevBuf *d_range = range ? &s.buf(np * n_out * 2 * 8) : nullptr;
    DevBuf &d_cnt = family_counters(s, 6);
    LawGapArgs a{};
    a.nt = n_t; a.m_max = pair_rows; a.n_out = n_out; a.n_pairs = n_pairs;
    a.row_off = d.off.as<long long>(); a.ef = d.ef.as<double>(); a.laws = d_laws.as<double>(); a.xs = d_xs.as<double>();
    a.pair_a = d_pa.as<int32_t>(); a.pair_b = d_pb.as<int32_t>(); a.tol = tol;
    a.radius = d_r.as<double>(); a.gap = d_g.as<double>(); a.witness = d_w.as<double>(); a.range = d_range ? d_range->as<double>() : nullptr;
    a.gap_row = d_row.as<int32_t>(); a.flag = d_f.as<int32_t>(); a.counters = d_cnt.as<unsigned long long>();
    family_launch(s, k_law_gap, n_pairs, lds, a);
    s.download(radius, d_r, np * 8);
    s.download(gap, d_g, np * 8);
    s.download(gap_row, d_row, np * 4);
    s.download(witness, d_w, np * n_t * 8);
    if (range) s.download(range, *d_range, np * n_out * 2 * 8);
    s.download(flag, d_f, np * 4);
    return family_close(s, d_cnt, 6, stats, ms);
}

// ---- the candidate sweep and the row screen (box_pairs.hpp) -----------------------------------------------------------
template <bool EMIT> static void box_pairs_launch(dim3 grid, const BoxPairArgs &a) {
    if (a.nt <= 4) hipLaunchKernelGGL((k_box_pairs<4, EMIT>), grid, dim3(BP_BLOCK), 0, nullptr, a);
    else if (a.nt <= 8) hipLaunchKernelGGL((k_box_pairs<8, EMIT>), grid, dim3(BP_BLOCK), 0, nullptr, a);
    else hipLaunchKernelGGL((k_box_pairs<16, EMIT>), grid, dim3(BP_BLOCK), 0, nullptr, a);
}

extern "C" int mpc_box_pairs(int32_t device, int32_t n_t, int32_t mode, int64_t n_a, const double *box_a, const uint8_t *usable_a, int64_t n_b,
                             const double *box_b, const uint8_t *usable_b, double margin, int64_t i0, int64_t i1, int64_t cap, int64_t *pair_a,
                             int64_t *pair_b, int64_t *row_count, int64_t *total, int64_t *stats, float *ms) {
    const char *who = "mpc_box_pairs";
    family_open(stats, 3, ms);
    if (total) *total = 0;
    if (n_t < 1 || n_t > BP_MAX_NT) return bad(who, "n_t must lie in 1..16");
    if (mode != BP_CROSS && mode != BP_UPPER) return bad(who, "mode must be 0 (CROSS) or 1 (UPPER)");
    if (n_a < 1 || (mode == BP_CROSS && n_b < 1)) return bad(who, "a family has no box");
    if (!box_a || !usable_a || !total || (mode == BP_CROSS && (!box_b || !usable_b))) return bad(who, "missing array");
    if (mode == BP_UPPER) {
        if ((box_b && box_b != box_a) || (usable_b && usable_b != usable_a) || (n_b != n_a && n_b != 0))
            return bad(who, "UPPER takes one family against itself: leave family b out or pass family a again");
        n_b = n_a; box_b = box_a; usable_b = usable_a;
    }
    if (n_a > 0x7fffffffll || n_b > 0x7fffffffll) return bad(who, "too many boxes for one launch");
    if (i0 < 0 || i1 < i0 || i1 > n_a) return bad(who, "the row range must lie in 0 <= i0 <= i1 <= n_a");
    if (cap < 0) return bad(who, "cap must be >= 0");
    if (cap > 0 && (!pair_a || !pair_b)) return bad(who, "missing array (pair_a or pair_b with cap > 0)");
    if (!std::isfinite(margin)) return bad(who, "margin must be finite");
    const int64_t rows = i1 - i0;
    if (row_count) std::fill(row_count, row_count + rows, (int64_t)0);
    // the box tests of the range: usable a x usable b, for UPPER the usable j > i behind every usable i
    int64_t tests = 0, ua = 0, ub = 0;
    for (int64_t j = 0; j < n_b; ++j) ub += usable_b[j] != 0;
    if (mode == BP_CROSS) {
        for (int64_t i = i0; i < i1; ++i) ua += usable_a[i] != 0;
        tests = ua * ub;
    } else {
        int64_t behind = 0;
        for (int64_t i = n_a - 1; i >= i0; --i) {
            if (usable_a[i] && i < i1) tests += behind;
            behind += usable_a[i] != 0;
        }
    }
    if (stats) stats[0] = tests;
    if (tests == 0) return MPC_OK;      // a family (or the range) without a usable box: no pair, no launch
    if (int rc = select_device(nullptr, device)) return rc;
    const long long row_blocks = (rows + BP_BLOCK - 1) / BP_BLOCK, n_tiles = (n_b + BP_TILE - 1) / BP_TILE;
    // segments: about four workgroups per CU, at most BP_MAX_SEG, every one a whole number of tiles
    long long n_seg = std::min<long long>({n_tiles, (long long)BP_MAX_SEG, (4ll * std::max(1, cu_count(device)) + row_blocks - 1) / row_blocks});
    const long long seg_tiles = (n_tiles + n_seg - 1) / n_seg;
    n_seg = (n_tiles + seg_tiles - 1) / seg_tiles;
    const size_t n_cells = (size_t)rows * (size_t)n_seg, box_bytes_a = (size_t)n_a * 2 * n_t * 8, box_bytes_b = (size_t)n_b * 2 * n_t * 8;
    OneShot s(who, nullptr, true);
    DevBuf &d_ba = s.upload(box_a, box_bytes_a), &d_ua = s.upload(usable_a, (size_t)n_a);
    DevBuf &d_bb = mode == BP_UPPER ? d_ba : s.upload(box_b, box_bytes_b), &d_ub = mode == BP_UPPER ? d_ua : s.upload(usable_b, (size_t)n_b);
    DevBuf &d_cnt = s.buf((n_cells + 1) * 8), &d_off = s.buf((n_cells + 1) * 8);
    s.fill(d_cnt, 0, (n_cells + 1) * 8);    // the entry behind the last cell stays 0: the scan leaves the total there
    size_t tmp_bytes = 0;
    s.chk(rocprim::exclusive_scan(nullptr, tmp_bytes, d_cnt.as<unsigned long long>(), d_off.as<unsigned long long>(), 0ull, n_cells + 1,
                                  rocprim::plus<unsigned long long>(), nullptr));
    DevBuf &d_tmp = s.buf(std::max<size_t>(8, tmp_bytes));
    BoxPairArgs a{};
    a.nt = n_t; a.mode = mode; a.n_seg = (int)n_seg; a.seg_tiles = (int)seg_tiles; a.n_b = n_b; a.n_tiles = n_tiles; a.i0 = i0; a.rows = rows;
    a.box_a = d_ba.as<double>(); a.box_b = d_bb.as<double>(); a.usable_a = d_ua.as<uint8_t>(); a.usable_b = d_ub.as<uint8_t>();
    a.margin = margin; a.counts = d_cnt.as<unsigned long long>(); a.offsets = d_off.as<unsigned long long>();
    const dim3 grid((unsigned)row_blocks, (unsigned)n_seg);
    DevBuf *d_rc = row_count ? &s.buf((size_t)rows * 8) : nullptr;
    s.launch_timed([&] {
        box_pairs_launch<false>(grid, a);
        s.chk(rocprim::exclusive_scan(d_tmp.p, tmp_bytes, d_cnt.as<unsigned long long>(), d_off.as<unsigned long long>(), 0ull, n_cells + 1,
                                      rocprim::plus<unsigned long long>(), nullptr));
        if (d_rc && s.ok())
            hipLaunchKernelGGL(k_box_row_counts, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, nullptr, (long long)rows, (int)n_seg,
                               d_off.as<unsigned long long>(), d_rc->as<long long>());
    });
    unsigned long long n_pairs = 0;
    s.download(&n_pairs, DevBuf{d_off.as<unsigned long long>() + n_cells, 8}, 8);    // a blocking copy: the count pass has ended
    if (d_rc) s.download(row_count, *d_rc, (size_t)rows * 8);
    float ms_count = 0.0f, ms_emit = 0.0f;
    s.elapsed(&ms_count);
    if (!s.ok()) return s.finish();
    *total = (int64_t)n_pairs;
    if (stats) { stats[1] = (int64_t)n_pairs; stats[2] = n_seg; }
    if (cap > 0 && n_pairs > 0 && n_pairs <= (unsigned long long)cap) {      // a list that does not fit is not written at all
        DevBuf &d_pa = s.buf((size_t)n_pairs * 8), &d_pb = s.buf((size_t)n_pairs * 8);
        a.pair_a = d_pa.as<long long>(); a.pair_b = d_pb.as<long long>();
        s.launch_timed([&] { box_pairs_launch<true>(grid, a); });
        s.download(pair_a, d_pa, (size_t)n_pairs * 8);
        s.download(pair_b, d_pb, (size_t)n_pairs * 8);
        s.elapsed(&ms_emit);
    }
    if (ms) *ms = ms_count + ms_emit;
    return s.finish();
}

extern "C" int mpc_pair_screen(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, int64_t n_pairs,
                               const int64_t *pair_a, const int64_t *pair_b, const double *box_for_a_rows, const double *box_for_b_rows,
                               int32_t sides, uint8_t *keep, int64_t *stats, float *ms) {
    const char *who = "mpc_pair_screen";
    family_open(stats, 3, ms);
    int m_max = 1;
    if (int rc = merge_check(who, n_t, n_regions, row_off, ef_rows, &m_max)) return rc;
    if (int rc = check_count(who, "n_pairs", n_pairs)) return rc;
    if (sides < 1 || sides > (PS_SIDE_A | PS_SIDE_B)) return bad(who, "sides must be 1 (rows of a), 2 (rows of b) or 3 (both)");
    if (n_pairs == 0) return MPC_OK;
    if (!pair_a || !pair_b || !keep || ((sides & PS_SIDE_A) && !box_for_a_rows) || ((sides & PS_SIDE_B) && !box_for_b_rows)) return bad(who, "missing array");
    for (int64_t k = 0; k < n_pairs; ++k)
        if (pair_a[k] < 0 || pair_a[k] >= n_regions || pair_b[k] < 0 || pair_b[k] >= n_regions) return bad(who, "a pair names a region out of range");
    if (int rc = select_device(nullptr, device)) return rc;
    const size_t np = (size_t)n_pairs, box_bytes = (size_t)n_regions * 2 * n_t * 8;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_regions, row_off, ef_rows, n_t + 1);
    DevBuf &d_pa = s.upload(pair_a, np * 8), &d_pb = s.upload(pair_b, np * 8);
    DevBuf *d_xa = (sides & PS_SIDE_A) ? &s.upload(box_for_a_rows, box_bytes) : nullptr;
    DevBuf *d_xb = !(sides & PS_SIDE_B) ? nullptr : (box_for_b_rows == box_for_a_rows && d_xa) ? d_xa : &s.upload(box_for_b_rows, box_bytes);
    DevBuf &d_keep = s.buf(np), &d_cnt = family_counters(s, 3);
    PairScreenArgs a{};
    a.nt = n_t; a.sides = sides; a.n_pairs = n_pairs; a.row_off = d.off.as<long long>(); a.ef = d.ef.as<double>();
    a.pair_a = d_pa.as<long long>(); a.pair_b = d_pb.as<long long>();
    a.box_for_a = d_xa ? d_xa->as<double>() : nullptr; a.box_for_b = d_xb ? d_xb->as<double>() : nullptr;
    a.keep = d_keep.as<uint8_t>(); a.counters = d_cnt.as<unsigned long long>();
    const dim3 grid((unsigned)((n_pairs + 255) / 256));
    s.launch_timed([&] {
        if (n_t <= 4) hipLaunchKernelGGL(k_pair_screen<4>, grid, dim3(256), 0, nullptr, a);
        else if (n_t <= 8) hipLaunchKernelGGL(k_pair_screen<8>, grid, dim3(256), 0, nullptr, a);
        else hipLaunchKernelGGL(k_pair_screen<16>, grid, dim3(256), 0, nullptr, a);
    });
    s.download(keep, d_keep, np);
    return family_close(s, d_cnt, 3, stats, ms);
}

// ---- transition graph of a closed loop (transition.hpp) ---------------------------------------------------------------
// Phi [n_regions][n_t][n_t], phi and, with want_xs, xs [n_regions][n_t]: present and finite
static int transition_check_maps(const char *who, int32_t n_t, int64_t n_regions, const double *Phi, const double *phi, bool want_xs,
                                 const double *xs) {
    if (n_regions == 0) return MPC_OK;
    if (!Phi || !phi || (want_xs && !xs)) return bad(who, want_xs ? "missing array (Phi, phi or xs)" : "missing array (Phi or phi)");
    if (int rc = check_finite(who, "Phi", Phi, n_regions * n_t * n_t)) return rc;
    const char *name = want_xs ? "phi and xs" : "phi";
    if (int rc = check_finite(who, name, phi, n_regions * n_t)) return rc;
    return want_xs ? check_finite(who, name, xs, n_regions * n_t) : (int)MPC_OK;
}

extern "C" int mpc_transition_boxes(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *Phi,
                                    const double *phi, const double *xs, double *image_box, int32_t *flag, int64_t *stats, float *ms) {
    const char *who = "mpc_transition_boxes";
    family_open(stats, 3, ms);
    int m_max = 1;
    if (int rc = merge_check(who, n_t, n_regions, row_off, ef_rows, &m_max)) return rc;
    if (int rc = transition_check_maps(who, n_t, n_regions, Phi, phi, true, xs)) return rc;
    if (n_regions == 0) return MPC_OK;
    if (!image_box || !flag) return bad(who, "missing output array");
    if (int rc = select_device(nullptr, device)) return rc;
    const size_t nr = (size_t)n_regions;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_regions, row_off, ef_rows, n_t + 1);
    DevBuf &d_Phi = s.upload(Phi, nr * n_t * n_t * 8), &d_phi = s.upload(phi, nr * n_t * 8), &d_xs = s.upload(xs, nr * n_t * 8);
    DevBuf &d_box = s.buf(nr * 2 * n_t * 8), &d_f = s.buf(nr * 4), &d_cnt = family_counters(s, 3);
    family_launch(s, k_transition_boxes, n_regions, tr_lds_bytes(m_max, n_t), (int)n_t, m_max, (long long)n_regions, d.off.as<long long>(),
                  d.ef.as<double>(), d_Phi.as<double>(), d_phi.as<double>(), d_xs.as<double>(), d_box.as<double>(), d_f.as<int32_t>(),
                  d_cnt.as<unsigned long long>());
    s.download(image_box, d_box, nr * 2 * n_t * 8);
    s.download(flag, d_f, nr * 4);
    return family_close(s, d_cnt, 3, stats, ms);
}

extern "C" int mpc_transition_pairs(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *Phi,
                                    const double *phi, const double *xs, int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b,
                                    int32_t full_radius, double tol, double *radius, int32_t *status, double *witness, int64_t *stats, float *ms) {
    const char *who = "mpc_transition_pairs";
    family_open(stats, 4, ms);
    int m_max = 1;
    if (int rc = merge_check(who, n_t, n_regions, row_off, ef_rows, &m_max)) return rc;
    if (int rc = check_tol(who, tol)) return rc;
    if (int rc = check_count(who, "n_pairs", n_pairs)) return rc;
    if (int rc = transition_check_maps(who, n_t, n_regions, Phi, phi, true, xs)) return rc;
    if (n_pairs == 0) return MPC_OK;
    if (!pair_a || !pair_b || !radius || !status || !witness) return bad(who, "missing array");
    int pair_rows = 2;     // p == q is a self loop
    if (int rc = check_indices(who, "a pair names a region out of range", n_pairs, {{pair_a, n_regions, row_off}, {pair_b, n_regions, row_off}}, false,
                               0, &pair_rows)) return rc;
    if (int rc = select_device(nullptr, device)) return rc;
    const size_t lds = tr_lds_bytes(pair_rows, n_t);   // 512 rows at n_t = 16: 78,840 bytes
    const size_t np = (size_t)n_pairs, nr = (size_t)n_regions;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_regions, row_off, ef_rows, n_t + 1);
    DevBuf &d_Phi = s.upload(Phi, nr * n_t * n_t * 8), &d_phi = s.upload(phi, nr * n_t * 8), &d_xs = s.upload(xs, nr * n_t * 8);
    DevBuf &d_pa = s.upload(pair_a, np * 4), &d_pb = s.upload(pair_b, np * 4);
    DevBuf &d_r = s.buf(np * 8), &d_st = s.buf(np * 4), &d_w = s.buf(np * n_t * 8), &d_cnt = family_counters(s, 4);
    TransitionPairArgs a{};
    a.nt = n_t; a.m_max = pair_rows; a.full_radius = full_radius ? 1 : 0; a.n_pairs = n_pairs;
    a.row_off = d.off.as<long long>(); a.ef = d.ef.as<double>(); a.Phi = d_Phi.as<double>(); a.phi = d_phi.as<double>();
    a.xs = d_xs.as<double>(); a.pair_a = d_pa.as<int32_t>(); a.pair_b = d_pb.as<int32_t>(); a.tol = tol;
    a.radius = d_r.as<double>(); a.witness = d_w.as<double>(); a.status = d_st.as<int32_t>();
    a.counters = d_cnt.as<unsigned long long>();
    family_launch(s, k_transition_pairs, n_pairs, lds, a);
    s.download(radius, d_r, np * 8);
    s.download(status, d_st, np * 4);
    s.download(witness, d_w, np * n_t * 8);
    return family_close(s, d_cnt, 4, stats, ms);
}

// ---- exit sets of a closed loop (exit_sets.hpp) -------------------------------------------------------------------------
extern "C" int mpc_exit_split(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *Phi,
                              const double *phi, int64_t n_pieces, const int64_t *piece_off, const double *piece_rows, int64_t n_items,
                              const int32_t *item_piece, const int32_t *item_source, const int32_t *item_target, const double *start, double tol,
                              int32_t *flag, uint64_t *mask, int64_t *stats, float *ms) {
    const char *who = "mpc_exit_split";
    family_open(stats, 5, ms);
    int m_reg = 1, m_piece = 1;
    if (int rc = merge_check(who, n_t, n_regions, row_off, ef_rows, &m_reg)) return rc;
    if (int rc = merge_check("mpc_exit_split (pieces)", n_t, n_pieces, piece_off, piece_rows, &m_piece)) return rc;
    if (int rc = check_tol(who, tol)) return rc;
    if (int rc = check_count(who, "n_items", n_items)) return rc;
    if (int rc = transition_check_maps(who, n_t, n_regions, Phi, phi, false, nullptr)) return rc;
    if (n_items == 0) return MPC_OK;
    if (!item_piece || !item_source || !item_target || !flag || !mask) return bad(who, "missing array");
    int item_rows = 4;     // source == target: the piece minus the part that stays in its region
    if (int rc = check_indices(who, "an item names a piece or a region out of range", n_items,
                               {{item_piece, n_pieces, piece_off}, {item_source, n_regions, nullptr}, {item_target, n_regions, row_off}}, false, 0,
                               &item_rows)) return rc;
    if (start)
        if (int rc = check_finite(who, "start", start, n_items * n_t)) return rc;
    if (int rc = select_device(nullptr, device)) return rc;
    const size_t lds = tr_lds_bytes(item_rows, n_t);   // 512 rows at n_t = 16: 78,840 bytes (the static s_mask adds 32)
    const size_t ni = (size_t)n_items, nr = (size_t)n_regions, words = ni * OV_WORDS * 8;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_regions, row_off, ef_rows, n_t + 1);
    const RegionsOnDevice pc = upload_regions(s, n_pieces, piece_off, piece_rows, n_t + 1);
    DevBuf &d_Phi = s.upload(Phi, nr * n_t * n_t * 8), &d_phi = s.upload(phi, nr * n_t * 8);
    DevBuf &d_ip = s.upload(item_piece, ni * 4), &d_is = s.upload(item_source, ni * 4), &d_it = s.upload(item_target, ni * 4);
    DevBuf *d_start = start ? &s.upload(start, ni * n_t * 8) : nullptr;
    DevBuf &d_f = s.buf(ni * 4), &d_m = s.buf(words), &d_cnt = family_counters(s, 5);
    ExitSplitArgs a{};
    a.nt = n_t; a.m_max = item_rows; a.n_items = n_items;
    a.row_off = d.off.as<long long>(); a.ef = d.ef.as<double>(); a.piece_off = pc.off.as<long long>(); a.piece_ef = pc.ef.as<double>();
    a.Phi = d_Phi.as<double>(); a.phi = d_phi.as<double>();
    a.item_piece = d_ip.as<int32_t>(); a.item_source = d_is.as<int32_t>(); a.item_target = d_it.as<int32_t>();
    a.start = d_start ? d_start->as<double>() : nullptr; a.tol = tol;
    a.flag = d_f.as<int32_t>(); a.mask = d_m.as<unsigned long long>(); a.counters = d_cnt.as<unsigned long long>();
    family_launch(s, k_exit_split, n_items, lds, a);
    s.download(flag, d_f, ni * 4);
    s.download(mask, d_m, words);
    return family_close(s, d_cnt, 5, stats, ms);
}

// ---- redundant rows of polytopes (reduce.hpp) ---------------------------------------------------------------------------
extern "C" int mpc_reduce_rows(int32_t device, int32_t n_t, int64_t n_poly, const int64_t *row_off, const double *ef_rows, const double *start,
                               double tol, int32_t *status, int32_t *wide, uint64_t *kept, double *point, int64_t *stats, float *ms) {
    const char *who = "mpc_reduce_rows";
    family_open(stats, 5, ms);
    int m_max = 1;
    if (int rc = merge_check(who, n_t, n_poly, row_off, ef_rows, &m_max, RD_MAX_ROWS)) return rc;
    if (int rc = check_tol(who, tol)) return rc;
    if (n_poly == 0) return MPC_OK;
    if (!status || !wide || !kept) return bad(who, "missing array");
    if (start)
        if (int rc = check_finite(who, "start", start, n_poly * n_t)) return rc;
    if (int rc = select_device(nullptr, device)) return rc;
    const size_t lds = tr_lds_bytes(m_max, n_t);   // 512 rows at n_t = 16: 78,840 bytes (the static s_kept adds 64)
    const size_t np = (size_t)n_poly, words = np * RD_WORDS * 8;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_poly, row_off, ef_rows, n_t + 1);
    DevBuf *d_start = start ? &s.upload(start, np * n_t * 8) : nullptr, *d_point = point ? &s.buf(np * n_t * 8) : nullptr;
    DevBuf &d_st = s.buf(np * 4), &d_w = s.buf(np * 4), &d_k = s.buf(words), &d_cnt = family_counters(s, 5);
    ReduceArgs a{};
    a.nt = n_t; a.m_max = m_max; a.n_poly = n_poly;
    a.row_off = d.off.as<long long>(); a.ef = d.ef.as<double>(); a.start = d_start ? d_start->as<double>() : nullptr; a.tol = tol;
    a.status = d_st.as<int32_t>(); a.wide = d_w.as<int32_t>(); a.kept = d_k.as<unsigned long long>();
    a.point = d_point ? d_point->as<double>() : nullptr; a.counters = d_cnt.as<unsigned long long>();
    family_launch(s, k_reduce_rows, n_poly, lds, a);
    s.download(status, d_st, np * 4);
    s.download(wide, d_w, np * 4);
    s.download(kept, d_k, words);
    if (point) s.download(point, *d_point, np * n_t * 8);
    return family_close(s, d_cnt, 5, stats, ms);
}

// ---- support functions of polytopes (support.hpp) -------------------------------------------------------------------------
extern "C" int mpc_support_rows(int32_t device, int32_t n_t, int64_t n_poly, const int64_t *row_off, const double *ef_rows, const int64_t *dir_off,
                                const double *dirs, const double *start, double tol, double *value, double *arg, int32_t *dir_status,
                                int32_t *poly_status, int32_t *wide, double *point, int64_t *stats, float *ms) {
    const char *who = "mpc_support_rows";
    family_open(stats, 7, ms);
    int m_max = 1;
    if (int rc = merge_check(who, n_t, n_poly, row_off, ef_rows, &m_max, RD_MAX_ROWS)) return rc;
    if (int rc = check_tol(who, tol)) return rc;
    if (n_poly == 0) return MPC_OK;
    if (!dir_off) return bad(who, "missing dir_off");
    if (dir_off[0] != 0) return bad(who, "dir_off[0] must be 0");
    // the items: polytope q's directions in blocks of SF_BLOCK, one item for a polytope without any
    std::vector<int32_t> item_poly, item_count;
    std::vector<long long> item_first;
    for (int64_t q = 0; q < n_poly; ++q) {
        const int64_t k = dir_off[q + 1] - dir_off[q];
        if (k < 0) return bad(who, "dir_off decreases");
        if (dir_off[q + 1] > 0x7fffffffll) return bad(who, "more than 2^31 - 1 directions");
        for (int64_t j = 0; j == 0 || j < k; j += SF_BLOCK) {
            item_poly.push_back((int32_t)q);
            item_first.push_back(dir_off[q] + j);
            item_count.push_back((int32_t)std::min<int64_t>(SF_BLOCK, k - j));
        }
    }
    const int64_t n_dir = dir_off[n_poly], n_items = (int64_t)item_poly.size();
    if (int rc = check_count(who, "n_items", n_items)) return rc;
    if (!value || !dir_status || !poly_status || !wide || (n_dir > 0 && !dirs)) return bad(who, "missing array");
    if (int rc = check_finite(who, "dirs", dirs, n_dir * n_t)) return rc;
    if (start)
        if (int rc = check_finite(who, "start", start, n_poly * n_t)) return rc;
    if (int rc = select_device(nullptr, device)) return rc;
    const size_t lds = sf_lds_bytes(m_max, n_t);   // 512 rows at n_t = 16: 79,112 bytes
    const size_t np = (size_t)n_poly, nd = (size_t)n_dir, ni = (size_t)n_items;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_poly, row_off, ef_rows, n_t + 1);
    DevBuf &d_doff = s.upload(dir_off, (np + 1) * 8), &d_dirs = s.upload(dirs, nd * n_t * 8);
    DevBuf &d_ip = s.upload(item_poly.data(), ni * 4), &d_ic = s.upload(item_count.data(), ni * 4), &d_if = s.upload(item_first.data(), ni * 8);
    DevBuf *d_start = start ? &s.upload(start, np * n_t * 8) : nullptr, *d_point = point ? &s.buf(np * n_t * 8) : nullptr;
    DevBuf *d_arg = arg ? &s.buf(std::max<size_t>(8, nd * n_t * 8)) : nullptr;
    DevBuf &d_val = s.buf(std::max<size_t>(8, nd * 8)), &d_ds = s.buf(std::max<size_t>(8, nd * 4)), &d_ps = s.buf(np * 4), &d_w = s.buf(np * 4);
    DevBuf &d_cnt = family_counters(s, 7);
    SupportArgs a{};
    a.nt = n_t; a.m_max = m_max; a.n_items = n_items;
    a.row_off = d.off.as<long long>(); a.ef = d.ef.as<double>(); a.dir_off = d_doff.as<long long>(); a.dirs = d_dirs.as<double>();
    a.item_poly = d_ip.as<int32_t>(); a.item_count = d_ic.as<int32_t>(); a.item_first = d_if.as<long long>();
    a.start = d_start ? d_start->as<double>() : nullptr; a.tol = tol;
    a.value = d_val.as<double>(); a.arg = d_arg ? d_arg->as<double>() : nullptr; a.dir_status = d_ds.as<int32_t>();
    a.poly_status = d_ps.as<int32_t>(); a.wide = d_w.as<int32_t>(); a.point = d_point ? d_point->as<double>() : nullptr;
    a.counters = d_cnt.as<unsigned long long>();
    family_launch(s, k_support_rows, n_items, lds, a);
    s.download(value, d_val, nd * 8);
    if (arg) s.download(arg, *d_arg, nd * n_t * 8);
    s.download(dir_status, d_ds, nd * 4);
    s.download(poly_status, d_ps, np * 4);
    s.download(wide, d_w, np * 4);
    if (point) s.download(point, *d_point, np * n_t * 8);
    return family_close(s, d_cnt, 7, stats, ms);
}

// ---- projections of polytopes (project.hpp) ------------------------------------------------------------------------------
extern "C" int mpc_project_rows(int32_t device, int32_t n, int32_t n_elim, int64_t n_poly, const int64_t *row_off, const double *ef_rows,
                                const double *start, double tol, int32_t out_cap, double *out_rows, int32_t *n_out, int32_t *status, int32_t *wide,
                                int32_t *peak, double *point, int64_t *stats, float *ms) {
    const char *who = "mpc_project_rows";
    family_open(stats, 9, ms);
    int m_max = 1;
    if (int rc = merge_check(who, n, n_poly, row_off, ef_rows, &m_max, PJ_MAX_ROWS)) return rc;
    if (n_elim < 0 || n_elim > n - 1) return bad(who, "n_elim must lie in 0..n - 1");
    if (int rc = check_tol(who, tol)) return rc;
    if (out_cap < 1 || out_cap > PJ_MAX_ROWS) return bad(who, "out_cap must lie in 1.." + std::to_string(PJ_MAX_ROWS));
    if (n_poly == 0) return MPC_OK;
    if (!out_rows || !n_out || !status || !wide) return bad(who, "missing array");
    if (start)
        if (int rc = check_finite(who, "start", start, n_poly * n)) return rc;
    if (int rc = select_device(nullptr, device)) return rc;
    // The rows of each LDS area: what a step of an item can make.  One step makes |Z| + |P||N| <= max(m, m^2 / 4) rows of m; the rows
    // a second step starts from are known on the device alone, so two steps or more take the limit.
    const int m_lds = n_elim == 0 ? m_max : n_elim == 1 ? std::min(PJ_MAX_ROWS, std::max(m_max, (m_max / 2) * ((m_max + 1) / 2))) : PJ_MAX_ROWS;
    const size_t lds = pj_lds_bytes(m_lds, n);   // 512 rows at n = 16: 148,472 bytes (the static arrays add 2,112)
    const int k = n - n_elim;
    const size_t np = (size_t)n_poly, out_bytes = np * (size_t)out_cap * (k + 1) * 8;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_poly, row_off, ef_rows, n + 1);
    DevBuf *d_start = start ? &s.upload(start, np * n * 8) : nullptr, *d_point = point ? &s.buf(np * k * 8) : nullptr, *d_peak = &s.buf(np * 4);
    DevBuf &d_out = s.buf(out_bytes), &d_no = s.buf(np * 4), &d_st = s.buf(np * 4), &d_w = s.buf(np * 4), &d_cnt = family_counters(s, 9);
    s.fill(d_out, 0, out_bytes);                   // the rows behind n_out[q] are zero
    if (point) s.fill(*d_point, 0, np * k * 8);   // an item without a result writes no point
    ProjectArgs a{};
    a.n = n; a.n_elim = n_elim; a.m_lds = m_lds; a.out_cap = out_cap; a.n_poly = n_poly;
    a.row_off = d.off.as<long long>(); a.ef = d.ef.as<double>(); a.start = d_start ? d_start->as<double>() : nullptr; a.tol = tol;
    a.status = d_st.as<int32_t>(); a.n_out = d_no.as<int32_t>(); a.wide = d_w.as<int32_t>(); a.peak = d_peak->as<int32_t>();
    a.out_rows = d_out.as<double>(); a.point = d_point ? d_point->as<double>() : nullptr; a.counters = d_cnt.as<unsigned long long>();
    family_launch(s, k_project_rows, n_poly, lds, a);
    s.download(status, d_st, np * 4);
    s.download(n_out, d_no, np * 4);
    s.download(wide, d_w, np * 4);
    if (peak) s.download(peak, *d_peak, np * 4);
    s.download(out_rows, d_out, out_bytes);
    if (point) s.download(point, *d_point, np * k * 8);
    return family_close(s, d_cnt, 9, stats, ms);
}

// ---- the cell table of the two calls that loop: backward exit cells and forward cells ---------------------------
// Both keep the cells of all steps in one CSR table that stays on the device and grows step by step; per step the item list goes up,
// status and n_kept come down, the host scans the offsets and lists the next items.  What the two do alike is here once: the argument
// checks, the table with its host and device side, the item list, the scan, the append, and the two ways out.  Each call keeps its own
// loop, launches and stop rules.

// What differs in the argument checks of a call: the names in its refusals, its own null checks, the start points it takes.
struct CellCall {
    const char *who, *who_cells;          // "mpc_x", "mpc_x (cells)"
    const char *adj, *adj_noun;           // "pred", "predecessor": <adj>_off, <adj>_idx, "a <adj_noun> list ..."
    const char *no_outputs;               // the refusal of a missing scalar output
    const char *cell0, *cell_noun;        // "missing <cell0>", "a cell names a <cell_noun> out of range"
    bool has_outputs, has_cell0, has_arrays;      // the scalar outputs, the per-cell inputs of step 0, the output arrays: all there
    bool want_xs;
    const double *xs, *cell_point0;       // [n_regions][n_t] with want_xs; [n_cells0][n_t] or nullptr: the call takes none
};

static int cells_check(const CellCall &c, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *Phi,
                       const double *phi, const int64_t *adj_off, const int32_t *adj_idx, int64_t n_cells0, const int64_t *cell_off0,
                       const double *cell_rows0, const int32_t *cell_reg0, double tol, int32_t max_steps, int64_t max_cells, int64_t max_rows_total) {
    const char *who = c.who;
    int m_reg = 1, m_cell = 1;
    if (int rc = merge_check(who, n_t, n_regions, row_off, ef_rows, &m_reg)) return rc;
    if (int rc = merge_check(c.who_cells, n_t, n_cells0, cell_off0, cell_rows0, &m_cell)) return rc;
    if (int rc = check_tol(who, tol)) return rc;
    if (int rc = transition_check_maps(who, n_t, n_regions, Phi, phi, c.want_xs, c.xs)) return rc;
    if (max_steps < 0) return bad(who, "max_steps must be >= 0");
    if (max_cells < 0 || max_cells > 0x7fffffffll || max_rows_total < 0) return bad(who, "max_cells must lie in 0..2^31 - 1 and max_rows_total be >= 0");
    if (!c.has_outputs) return bad(who, c.no_outputs);
    if (n_regions > 0) {
        if (!adj_off || adj_off[0] != 0) return bad(who, std::string(c.adj) + "_off must start at 0");
        for (int64_t i = 0; i < n_regions; ++i)
            if (adj_off[i + 1] < adj_off[i]) return bad(who, std::string(c.adj) + "_off must not decrease");
        if (adj_off[n_regions] > 0 && !adj_idx) return bad(who, std::string("missing ") + c.adj + "_idx");
        for (int64_t k = 0; k < adj_off[n_regions]; ++k)
            if (adj_idx[k] < 0 || adj_idx[k] >= n_regions) return bad(who, std::string("a ") + c.adj_noun + " list names a region out of range");
    }
    if (n_cells0 > 0) {
        if (!c.has_cell0) return bad(who, std::string("missing ") + c.cell0);
        for (int64_t k = 0; k < n_cells0; ++k)
            if (cell_reg0[k] < 0 || cell_reg0[k] >= n_regions) return bad(who, std::string("a cell names a ") + c.cell_noun + " out of range");
        if (c.cell_point0)
            if (int rc = check_finite(who, "cell_point0", c.cell_point0, n_cells0 * n_t)) return rc;
        if (n_cells0 > max_cells || cell_off0[n_cells0] > max_rows_total) return bad(who, "the cells of step 0 exceed max_cells or max_rows_total");
        if (!c.has_arrays) return bad(who, "missing output array");
    }
    return MPC_OK;
}

// b grown to ``bytes`` with what it holds kept: for a table of all steps
static void grow_kept(OneShot &s, DevBuf &b, size_t bytes) { if (s.ok()) s.chk(b.ensure(bytes, s.st, true)); }

// where a call wants the host's side of the table
struct CellOut { int64_t *n_cells; int32_t *status, *steps; int64_t *cell_off; int32_t *cell_reg, *cell_step, *cell_parent, *cell_wide; };

struct CellTable {
    const int n_t;
    const int64_t n_cells0;
    // the host's side: everything but the rows, the points and what else a call keeps per cell
    std::vector<int64_t> off;
    std::vector<int32_t> reg, stp, par, wid;      // reg: the source region (backward) or the region (forward) of a cell
    int64_t lo = 0, hi;                           // the cells of the last completed step
    // the device's side (to_device): offsets, rows [.][n_t + 1] and points [cells][n_t] of all steps; the items, the new cells' items, and
    // per item what the cell kernel writes: status, n_kept, kept [RD_WORDS], point [n_t]
    DevBuf *d_off = nullptr, *d_rows = nullptr, *d_pt = nullptr;
    DevBuf *d_ir = nullptr, *d_ic = nullptr, *d_ci = nullptr, *d_st = nullptr, *d_nk = nullptr, *d_kept = nullptr, *d_ipt = nullptr;
    // the items of the next step (list_items); what came down for them, and the new cells in item order (scan)
    std::vector<int32_t> item_region, item_cell, st, nk, cell_item;
    int item_rows = 2;                            // the LDS rows of the largest item
    bool too_many = false, fat = false;           // more than 2^31 - 1 items; a new cell with no row or more than OV_MAX_ROWS
    int64_t new_rows = 0;

    CellTable(int n_t_, int64_t n0, const int64_t *cell_off0, const int32_t *cell_reg0) : n_t(n_t_), n_cells0(n0), off(1, 0), hi(n0) {
        if (n0 > 0) {
            off.assign(cell_off0, cell_off0 + n0 + 1);
            reg.assign(cell_reg0, cell_reg0 + n0);
            stp.assign((size_t)n0, 0);
            par.assign((size_t)n0, -1);
            wid.assign((size_t)n0, 0);
        }
    }
    size_t row_bytes() const { return (size_t)off.back() * ((size_t)n_t + 1) * 8; }

    // cells_per_step [max_steps + 1] and step_ms [max_steps] before the first step
    void open_steps(int64_t *cells_per_step, float *step_ms, int max_steps) const {
        if (cells_per_step) {
            for (int k = 0; k <= max_steps; ++k) cells_per_step[k] = 0;
            cells_per_step[0] = n_cells0;
        }
        if (step_ms) for (int k = 0; k < max_steps; ++k) step_ms[k] = 0.0f;
    }

    // cell_point0 == nullptr: the cells of step 0 have no point
    void to_device(OneShot &s, const double *cell_rows0, const double *cell_point0) {
        const size_t pt_bytes = (size_t)n_cells0 * n_t * 8;
        d_off = &s.upload(off.data(), off.size() * 8);
        d_rows = &s.upload(cell_rows0, row_bytes());
        d_pt = cell_point0 ? &s.upload(cell_point0, pt_bytes) : &s.buf(pt_bytes);
        d_ir = &s.buf(); d_ic = &s.buf(); d_ci = &s.buf(); d_st = &s.buf(); d_nk = &s.buf(); d_kept = &s.buf(); d_ipt = &s.buf();
    }

    // The items of the next step: by parent cell of the last step, then as the adjacency list of its region is.  Both operands of an item
    // passed merge_check at MG_MAX_ROWS, so item_rows fits the row loop.
    static_assert(2 * MG_MAX_ROWS <= RD_MAX_ROWS, "an item's rows must fit rd_row_loop");
    void list_items(const int64_t *adj_off, const int32_t *adj_idx, const int64_t *row_off) {
        item_region.clear();
        item_cell.clear();
        item_rows = 2;
        too_many = false;
        for (int64_t c = lo; c < hi && !too_many; ++c) {
            const int64_t i = reg[(size_t)c], m_q = off[(size_t)c + 1] - off[(size_t)c];
            for (int64_t k = adj_off[i]; k < adj_off[i + 1]; ++k) {
                const int32_t j = adj_idx[k];
                item_region.push_back(j);
                item_cell.push_back((int32_t)c);
                item_rows = std::max<int>(item_rows, (int)(row_off[j + 1] - row_off[j] + m_q));
            }
            too_many = item_region.size() > 0x7fffffffull;
        }
    }

    // the item list up, room for what the cell kernel writes
    void upload_items(OneShot &s) {
        const size_t ni = item_region.size();
        s.upload(*d_ir, item_region.data(), ni * 4);
        s.upload(*d_ic, item_cell.data(), ni * 4);
        s.ensure(*d_st, ni * 4); s.ensure(*d_nk, ni * 4); s.ensure(*d_kept, ni * RD_WORDS * 8); s.ensure(*d_ipt, ni * n_t * 8);
    }

    // status and n_kept down, then the scan: the cells of this step in item order
    void scan(OneShot &s) {
        const size_t ni = item_region.size();
        st.resize(ni); nk.resize(ni);
        s.download(st.data(), *d_st, ni * 4);       // blocking copies on the null stream: the launch has ended
        s.download(nk.data(), *d_nk, ni * 4);
        cell_item.clear();
        new_rows = 0;
        fat = false;
        if (!s.ok()) return;
        for (size_t q = 0; q < ni; ++q) {
            if (st[q] != PC_CELL && st[q] != PC_CELL_WIDE) continue;
            fat = fat || nk[q] < 1 || nk[q] > OV_MAX_ROWS;
            cell_item.push_back((int32_t)q);
            new_rows += nk[q];
        }
    }

    // The caps on the scanned cells, in their one order; true and the call's own *code (for a fat cell, max_cells, max_rows_total) when
    // one refuses them.
    bool refused(int64_t max_cells, int64_t max_rows_total, int rows, int cells, int rows_total, int *code) const {
        if (cell_item.empty()) return false;
        if (fat) *code = rows;
        else if ((int64_t)(reg.size() + cell_item.size()) > max_cells) *code = cells;
        else if (off.back() + new_rows > max_rows_total) *code = rows_total;
        else return false;
        return true;
    }

    // The scanned cells join the table as step ``step``: the host's vectors, the device's tables grown with their contents kept, the
    // tail of the offsets and cell_item up.  Returns the first new cell; lo and hi stay until advance().
    size_t append(OneShot &s, int step) {
        const size_t nn = cell_item.size(), nc = reg.size();
        for (size_t c = 0; c < nn; ++c) {
            const size_t q = (size_t)cell_item[c], parent = (size_t)item_cell[q];
            off.push_back(off.back() + nk[q]);
            reg.push_back(item_region[q]);
            stp.push_back(step);
            par.push_back((int32_t)parent);
            wid.push_back(st[q] == PC_CELL_WIDE || wid[parent] ? 1 : 0);
        }
        grow_kept(s, *d_off, (nc + nn + 1) * 8);
        grow_kept(s, *d_rows, row_bytes());
        grow_kept(s, *d_pt, (nc + nn) * n_t * 8);
        if (s.ok()) s.chk(hipMemcpy(d_off->as<int64_t>() + nc + 1, off.data() + nc + 1, nn * 8, hipMemcpyHostToDevice));
        s.upload(*d_ci, cell_item.data(), nn * 4);
        return nc;
    }
    void advance() { lo = hi; hi = (int64_t)reg.size(); }

    void deliver(const CellOut &o, int code, int n_steps) const {
        const size_t nc = reg.size();
        *o.n_cells = (int64_t)nc;
        *o.status = code;
        *o.steps = n_steps;
        if (o.cell_off) std::memcpy(o.cell_off, off.data(), (nc + 1) * 8);
        if (nc) {
            std::memcpy(o.cell_reg, reg.data(), nc * 4);
            std::memcpy(o.cell_step, stp.data(), nc * 4);
            std::memcpy(o.cell_parent, par.data(), nc * 4);
            std::memcpy(o.cell_wide, wid.data(), nc * 4);
        }
    }

    // The closing download: the rows, the points of the cells from ``first_point`` on (cell_point == nullptr: none), the six counters to
    // stats; the call's code.
    int close(OneShot &s, const DevBuf &d_cnt, double *cell_rows, double *cell_point, size_t first_point, int64_t *stats) const {
        if (!s.ok()) return s.finish();
        const size_t nc = reg.size();
        s.download(cell_rows, *d_rows, row_bytes());
        if (cell_point && nc > first_point && s.ok())
            s.chk(hipMemcpy(cell_point + first_point * n_t, d_pt->as<double>() + first_point * n_t, (nc - first_point) * n_t * 8, hipMemcpyDeviceToHost));
        unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
        s.download(cnt, d_cnt, sizeof cnt);
        if (const int rc = s.finish()) return rc;
        if (stats) for (int i = 0; i < 6; ++i) stats[i] = (int64_t)cnt[i];
        return MPC_OK;
    }
};

// ---- backward exit cells of a closed loop (invariant.hpp) ---------------------------------------------------------------
extern "C" int mpc_backward_exits(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *Phi,
                                  const double *phi, const double *xs, const int64_t *pred_off, const int32_t *pred_idx, int64_t n_cells0,
                                  const int64_t *cell_off0, const double *cell_rows0, const int32_t *cell_source0, double tol, int32_t max_steps,
                                  int64_t max_cells, int64_t max_rows_total, int64_t *n_cells, int64_t *cell_off, double *cell_rows,
                                  int32_t *cell_source, int32_t *cell_step, int32_t *cell_parent, int32_t *cell_wide, double *cell_point,
                                  int32_t *status, int32_t *steps, int32_t *converged, int64_t *cells_per_step, float *step_ms, int64_t *stats,
                                  float *ms) {
    const char *who = "mpc_backward_exits";
    family_open(stats, 6, ms);
    if (n_cells) *n_cells = 0;
    if (steps) *steps = 0;
    if (converged) *converged = 0;
    if (status) *status = MPC_BACKWARD_MAX_STEPS;
    const CellCall call{who, "mpc_backward_exits (cells)", "pred", "predecessor", "missing output (n_cells, status, steps or converged)",
                        "cell_source0", "source region", n_cells && status && steps && converged, cell_source0 != nullptr,
                        cell_off && cell_rows && cell_source && cell_step && cell_parent && cell_wide, true, xs, nullptr};
    if (int rc = cells_check(call, n_t, n_regions, row_off, ef_rows, Phi, phi, pred_off, pred_idx, n_cells0, cell_off0, cell_rows0, cell_source0, tol,
                             max_steps, max_cells, max_rows_total))
        return rc;
    CellTable t(n_t, n_cells0, cell_off0, cell_source0);
    const CellOut out{n_cells, status, steps, cell_off, cell_source, cell_step, cell_parent, cell_wide};
    t.open_steps(cells_per_step, step_ms, max_steps);
    if (n_cells0 == 0 || max_steps == 0) {
        t.deliver(out, n_cells0 == 0 ? MPC_BACKWARD_CONVERGED : MPC_BACKWARD_MAX_STEPS, 0);
        *converged = n_cells0 == 0;
        if (n_cells0 > 0) std::memcpy(cell_rows, cell_rows0, t.row_bytes());
        return MPC_OK;
    }
    if (int rc = select_device(nullptr, device)) return rc;
    OneShot s(who, nullptr, true);
    const size_t nr = (size_t)n_regions;
    const RegionsOnDevice d = upload_regions(s, n_regions, row_off, ef_rows, n_t + 1);
    DevBuf &d_Phi = s.upload(Phi, nr * n_t * n_t * 8), &d_phi = s.upload(phi, nr * n_t * 8), &d_xs = s.upload(xs, nr * n_t * 8);
    t.to_device(s, cell_rows0, nullptr);
    DevBuf &d_cnt = family_counters(s, 6);
    int step = 0, code = MPC_BACKWARD_CONVERGED;
    float total_ms = 0.0f;
    for (;;) {
        t.list_items(pred_off, pred_idx, row_off);
        if (t.item_region.empty()) break;                                     // nothing can precede the last cells: converged
        if (step == max_steps) { code = MPC_BACKWARD_MAX_STEPS; break; }
        if (t.too_many) { code = MPC_BACKWARD_MAX_CELLS; break; }
        const size_t ni = t.item_region.size();
        const size_t lds = tr_lds_bytes(t.item_rows, n_t);   // 512 rows at n_t = 16: 78,840 bytes (the static s_kept adds 64)
        t.upload_items(s);
        PreCellArgs a{};
        a.nt = n_t; a.m_max = t.item_rows; a.n_items = (long long)ni;
        a.row_off = d.off.as<long long>(); a.ef = d.ef.as<double>(); a.cell_off = t.d_off->as<long long>(); a.cell_ef = t.d_rows->as<double>();
        a.Phi = d_Phi.as<double>(); a.phi = d_phi.as<double>(); a.xs = d_xs.as<double>();
        a.item_region = t.d_ir->as<int32_t>(); a.item_cell = t.d_ic->as<int32_t>(); a.tol = tol;
        a.status = t.d_st->as<int32_t>(); a.n_kept = t.d_nk->as<int32_t>(); a.kept = t.d_kept->as<unsigned long long>();
        a.point = t.d_ipt->as<double>(); a.counters = d_cnt.as<unsigned long long>();
        family_launch(s, k_pre_cells, (int64_t)ni, lds, a);
        t.scan(s);
        float t_cells = 0.0f, t_emit = 0.0f;
        s.elapsed(&t_cells);
        if (!s.ok()) break;
        const size_t nn = t.cell_item.size();
        const bool refused = t.refused(max_cells, max_rows_total, MPC_BACKWARD_ROWS, MPC_BACKWARD_MAX_CELLS, MPC_BACKWARD_MAX_ROWS_TOTAL, &code);
        if (nn && !refused) {
            const size_t nc = t.append(s, step + 1);
            PreEmitArgs e{};
            e.nt = n_t; e.m_max = t.item_rows; e.n_cells = (long long)nn; e.first_cell = (long long)nc;
            e.row_off = d.off.as<long long>(); e.cell_off = t.d_off->as<long long>(); e.ef = d.ef.as<double>(); e.cell_ef = t.d_rows->as<double>();
            e.Phi = d_Phi.as<double>(); e.phi = d_phi.as<double>(); e.item_region = t.d_ir->as<int32_t>(); e.item_cell = t.d_ic->as<int32_t>();
            e.cell_item = t.d_ci->as<int32_t>(); e.kept = t.d_kept->as<unsigned long long>(); e.point = t.d_ipt->as<double>();
            e.cell_point = t.d_pt->as<double>(); e.tol = tol;
            family_launch(s, k_pre_emit, (int64_t)nn, lds, e);
            if (s.ok()) s.chk(hipEventSynchronize(s.e1));
            s.elapsed(&t_emit);
            if (!s.ok()) break;
        }
        if (step_ms && step < max_steps) step_ms[step] = t_cells + t_emit;
        total_ms += t_cells + t_emit;
        if (!nn || refused) break;                                            // a step without a cell: converged
        ++step;
        if (cells_per_step) cells_per_step[step] = (int64_t)nn;
        t.advance();
    }
    if (int rc = t.close(s, d_cnt, cell_rows, cell_point, (size_t)n_cells0, stats)) return rc;
    if (ms) *ms = total_ms;
    t.deliver(out, code, step);
    *converged = code == MPC_BACKWARD_CONVERGED;
    return MPC_OK;
}

// ---- forward cells of a closed loop (forward.hpp) ---------------------------------------------------------------------
// Beside the cell table: the maps [G | g] and the regions of the cells on the device, and the points of step 0.
extern "C" int mpc_forward_cells(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *Phi,
                                 const double *phi, const int64_t *succ_off, const int32_t *succ_idx, int64_t n_cells0, const int64_t *cell_off0,
                                 const double *cell_rows0, const int32_t *cell_region0, const double *cell_point0, double tol, int32_t max_steps,
                                 int64_t max_cells, int64_t max_rows_total, int64_t *n_cells, int64_t *cell_off, double *cell_rows,
                                 int32_t *cell_region, int32_t *cell_step, int32_t *cell_parent, int32_t *cell_wide, double *cell_point,
                                 double *cell_map, int32_t *status, int32_t *steps, int64_t *cells_per_step, float *step_ms, int64_t *stats,
                                 float *ms) {
    const char *who = "mpc_forward_cells";
    family_open(stats, 6, ms);
    if (n_cells) *n_cells = 0;
    if (steps) *steps = 0;
    if (status) *status = MPC_FORWARD_DONE;
    const CellCall call{who, "mpc_forward_cells (cells)", "succ", "successor", "missing output (n_cells, status or steps)",
                        "cell_region0 or cell_point0", "region", n_cells && status && steps, cell_region0 && cell_point0,
                        cell_off && cell_rows && cell_region && cell_step && cell_parent && cell_wide && cell_point && cell_map, false, nullptr,
                        cell_point0};
    if (int rc = cells_check(call, n_t, n_regions, row_off, ef_rows, Phi, phi, succ_off, succ_idx, n_cells0, cell_off0, cell_rows0, cell_region0, tol,
                             max_steps, max_cells, max_rows_total))
        return rc;
    CellTable t(n_t, n_cells0, cell_off0, cell_region0);
    const CellOut out{n_cells, status, steps, cell_off, cell_region, cell_step, cell_parent, cell_wide};
    const size_t nr = (size_t)n_regions, w = (size_t)n_t + 1, map_doubles = (size_t)n_t * w;
    // step 0: theta_0 = I theta_0 + 0
    std::vector<double> map0((size_t)n_cells0 * map_doubles, 0.0);
    for (size_t c = 0; c < (size_t)n_cells0; ++c)
        for (int k = 0; k < n_t; ++k) map0[c * map_doubles + (size_t)k * w + k] = 1.0;
    t.open_steps(cells_per_step, step_ms, max_steps);
    if (n_cells0 == 0 || max_steps == 0) {
        t.deliver(out, n_cells0 == 0 ? MPC_FORWARD_EMPTY : MPC_FORWARD_DONE, 0);
        if (n_cells0 > 0) {
            std::memcpy(cell_rows, cell_rows0, t.row_bytes());
            std::memcpy(cell_point, cell_point0, (size_t)n_cells0 * n_t * 8);
            std::memcpy(cell_map, map0.data(), map0.size() * 8);
        }
        return MPC_OK;
    }
    if (int rc = select_device(nullptr, device)) return rc;
    OneShot s(who, nullptr, true);
    const RegionsOnDevice d = upload_regions(s, n_regions, row_off, ef_rows, n_t + 1);
    DevBuf &d_Phi = s.upload(Phi, nr * n_t * n_t * 8), &d_phi = s.upload(phi, nr * n_t * 8);
    t.to_device(s, cell_rows0, cell_point0);
    DevBuf &d_cmap = s.upload(map0.data(), map0.size() * 8), &d_creg = s.upload(t.reg.data(), t.reg.size() * 4), &d_cnt = family_counters(s, 6);
    DevBuf &d_next = s.buf();
    int step = 0, code = MPC_FORWARD_DONE;
    float total_ms = 0.0f;
    while (step < max_steps) {
        t.list_items(succ_off, succ_idx, row_off);
        if (t.item_region.empty()) { code = MPC_FORWARD_EMPTY; break; }        // no region follows the last cells: every trajectory has left
        if (t.too_many) { code = MPC_FORWARD_MAX_CELLS; break; }
        const size_t ni = t.item_region.size(), np = (size_t)(t.hi - t.lo);
        const size_t lds = tr_lds_bytes(t.item_rows, n_t);   // 512 rows at n_t = 16: 78,840 bytes (the static arrays add 2,528)
        float t_maps = 0.0f, t_cells = 0.0f, t_emit = 0.0f;
        t.upload_items(s);
        s.ensure(d_next, np * map_doubles * 8);
        family_launch(s, k_fwd_maps, (int64_t)np, 0, (int)n_t, (long long)np, (long long)t.lo, d_creg.as<int32_t>(), d_Phi.as<double>(),
                      d_phi.as<double>(), d_cmap.as<double>(), d_next.as<double>());
        if (s.ok()) s.chk(hipEventSynchronize(s.e1));
        s.elapsed(&t_maps);
        FwdCellArgs a{};
        a.nt = n_t; a.m_max = t.item_rows; a.n_items = (long long)ni; a.first = (long long)t.lo;
        a.row_off = d.off.as<long long>(); a.ef = d.ef.as<double>(); a.cell_off = t.d_off->as<long long>(); a.cell_ef = t.d_rows->as<double>();
        a.next = d_next.as<double>(); a.cell_point = t.d_pt->as<double>();
        a.item_region = t.d_ir->as<int32_t>(); a.item_cell = t.d_ic->as<int32_t>(); a.tol = tol;
        a.status = t.d_st->as<int32_t>(); a.n_kept = t.d_nk->as<int32_t>(); a.kept = t.d_kept->as<unsigned long long>();
        a.point = t.d_ipt->as<double>(); a.counters = d_cnt.as<unsigned long long>();
        family_launch(s, k_fwd_cells, (int64_t)ni, lds, a);
        t.scan(s);
        s.elapsed(&t_cells);
        if (!s.ok()) break;
        const size_t nn = t.cell_item.size();
        const bool refused = t.refused(max_cells, max_rows_total, MPC_FORWARD_ROWS, MPC_FORWARD_MAX_CELLS, MPC_FORWARD_MAX_ROWS_TOTAL, &code);
        if (nn && !refused) {
            const size_t nc = t.append(s, step + 1);
            grow_kept(s, d_cmap, (nc + nn) * map_doubles * 8);
            grow_kept(s, d_creg, (nc + nn) * 4);
            if (s.ok()) s.chk(hipMemcpy(d_creg.as<int32_t>() + nc, t.reg.data() + nc, nn * 4, hipMemcpyHostToDevice));
            FwdEmitArgs e{};
            e.nt = n_t; e.m_max = t.item_rows; e.n_cells = (long long)nn; e.first_cell = (long long)nc; e.first = (long long)t.lo;
            e.row_off = d.off.as<long long>(); e.cell_off = t.d_off->as<long long>(); e.ef = d.ef.as<double>(); e.cell_ef = t.d_rows->as<double>();
            e.next = d_next.as<double>(); e.cell_map = d_cmap.as<double>(); e.item_region = t.d_ir->as<int32_t>(); e.item_cell = t.d_ic->as<int32_t>();
            e.cell_item = t.d_ci->as<int32_t>(); e.kept = t.d_kept->as<unsigned long long>(); e.point = t.d_ipt->as<double>();
            e.cell_point = t.d_pt->as<double>(); e.tol = tol;
            family_launch(s, k_fwd_emit, (int64_t)nn, lds, e);
            if (s.ok()) s.chk(hipEventSynchronize(s.e1));
            s.elapsed(&t_emit);
            if (!s.ok()) break;
        }
        if (step_ms) step_ms[step] = t_maps + t_cells + t_emit;
        total_ms += t_maps + t_cells + t_emit;
        if (refused) break;
        if (!nn) { code = MPC_FORWARD_EMPTY; break; }                         // a step without a cell: every trajectory has left
        ++step;
        if (cells_per_step) cells_per_step[step] = (int64_t)nn;
        t.advance();
    }
    s.download(cell_map, d_cmap, t.reg.size() * map_doubles * 8);
    if (int rc = t.close(s, d_cnt, cell_rows, cell_point, 0, stats)) return rc;
    if (ms) *ms = total_ms;
    t.deliver(out, code, step);
    return MPC_OK;
}
