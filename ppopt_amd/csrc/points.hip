// points.hip -- programs solved at fixed points, one wavefront each: batched LPs (lp_batch.hpp: the deterministic-solver plug and
// the facet centres of the geometric algorithm) and the QP / MIQP of a program at parameter points (qp.hpp).  Nothing here looks
// inside an mpc_handle: every call is one OneShot (host_common.hpp) -- a batch in, one to three launches, the results out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mpcombi.h"
#include "lp_batch.hpp"
#include "qp.hpp"
#include "host_common.hpp"

using namespace mpc;

// ---- facet centres of a batch of polytopes (geometric algorithm) --------------------------------------------------------------
extern "C" int mpc_facet_centres(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, double *centre,
                                 double *radius, int32_t *status) {
    if (n_t < 1 || n_regions < 0 || !row_off || !centre || !radius || !status) return fail(nullptr, MPC_ERR_INVALID, "bad argument");
    const long long rows = n_regions ? row_off[n_regions] : 0;
    if (rows == 0) return MPC_OK;
    if (!ef_rows) return fail(nullptr, MPC_ERR_INVALID, "bad argument");
    if (int rc = select_device(nullptr, device)) return rc;
    int m_max = 0;
    std::vector<int32_t> reg((size_t)rows);
    for (long long r = 0; r < n_regions; ++r) {
        m_max = std::max<int>(m_max, (int)(row_off[r + 1] - row_off[r]));
        for (long long i = row_off[r]; i < row_off[r + 1]; ++i) reg[(size_t)i] = (int32_t)r;
    }
    const int n = n_t + 1, ld = odd_at_least(n + 3);
    const size_t lds = lp_lds_bytes(m_max + 1, ld);   // the region's rows and the row -r <= 0
    if (lds > 160 * 1024) return fail(nullptr, MPC_ERR_INVALID, "a region has too many rows for the 160 KiB LDS of one CU");
    if (lds > 48 * 1024) HIP_TRY(nullptr, hipFuncSetAttribute(reinterpret_cast<const void *>(k_facet_centres), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    OneShot s("mpc_facet_centres");
    DevBuf &d_ef = s.upload(ef_rows, (size_t)rows * (n_t + 1) * 8), &d_off = s.upload(row_off, (size_t)(n_regions + 1) * 8);
    DevBuf &d_reg = s.upload(reg.data(), (size_t)rows * 4);
    DevBuf &d_c = s.buf((size_t)rows * n_t * 8), &d_r = s.buf((size_t)rows * 8), &d_s = s.buf((size_t)rows * 4), &d_w = s.buf(256);
    s.fill(d_w, 0, 4);
    s.launch([&] {
        const int per_cu = std::max(1, std::min(32, (int)((160 * 1024) / lds)));
        const dim3 g((unsigned)std::min<long long>(rows, (long long)cu_count(device) * per_cu)), b(64);
        hipLaunchKernelGGL(k_facet_centres, g, b, lds, nullptr, rows, (int)n_t, m_max, ld, d_ef.as<double>(), d_off.as<long long>(), d_reg.as<int32_t>(),
                           d_c.as<double>(), d_r.as<double>(), d_s.as<int32_t>(), d_w.as<unsigned int>());
    });
    s.download(centre, d_c, (size_t)rows * n_t * 8);
    s.download(radius, d_r, (size_t)rows * 8);
    s.download(status, d_s, (size_t)rows * 4);
    return s.finish();
}

// ---- batched LPs ------------------------------------------------------------------------------------------------
int mpc::lp_batch(int32_t device, int64_t n_lp, int32_t m, int32_t n, const double *A, int32_t shared_A, const double *b, int32_t shared_b,
                  const double *c, int32_t shared_c, const uint8_t *eq, int32_t *status, double *x, double *obj, int32_t *iters, int32_t *tight) {
    if (n_lp < 0 || m < 1 || n < 1 || !A || !b || !eq || !status) return fail(nullptr, MPC_ERR_INVALID, "bad argument");
    if (n_lp == 0) return MPC_OK;
    if (int rc = select_device(nullptr, device)) return rc;
    const int ld = odd_at_least(n + 3);
    const size_t lds = lp_lds_bytes(m, ld);
    if (lds > 160 * 1024) return fail(nullptr, MPC_ERR_INVALID, "LP does not fit the 160 KiB LDS of one CU");
    if (lds > 48 * 1024) HIP_TRY(nullptr, hipFuncSetAttribute(reinterpret_cast<const void *>(k_lp_batch), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int n_cu = cu_count(device);
    const size_t szA = (shared_A ? 1 : (size_t)n_lp) * m * n * 8, szb = (shared_b ? 1 : (size_t)n_lp) * m * 8;
    const size_t szc = c ? (shared_c ? 1 : (size_t)n_lp) * n * 8 : 0;
    OneShot s("mpc_lp_solve_batch", OneShot::OwnStream{});
    DevBuf &d_A = s.upload(A, szA), &d_b = s.upload(b, szb), &d_c = c ? s.upload(c, szc) : s.buf(), &d_eq = s.upload(eq, (size_t)n_lp * m);
    // the kernel writes x, the objective and the pivot count of every LP, whether or not the caller takes them
    DevBuf &d_st = s.buf((size_t)n_lp * 4), &d_it = s.buf((size_t)n_lp * 4), &d_x = s.buf((size_t)n_lp * n * 8), &d_obj = s.buf((size_t)n_lp * 8);
    DevBuf &d_tight = s.buf(tight ? (size_t)n_lp * m * 4 : 0), &d_work = s.buf(4);
    s.fill(d_work, 0, 4);
    s.launch([&] {
        const int grid = (int)std::min<long long>(n_lp, (long long)std::max(n_cu, 1) * waves_per_cu((int)lds));
        hipLaunchKernelGGL(k_lp_batch, dim3(grid), dim3(64), lds, s.st, (long long)n_lp, m, n, ld, d_A.as<double>(), shared_A, d_b.as<double>(), shared_b,
                           d_c.as<double>(), shared_c, d_eq.as<uint8_t>(), d_st.as<int32_t>(), d_x.as<double>(), d_obj.as<double>(), d_it.as<int32_t>(),
                           d_tight.as<int32_t>(), d_work.as<unsigned int>());
    });
    s.download(status, d_st, (size_t)n_lp * 4);
    if (x) s.download(x, d_x, (size_t)n_lp * n * 8);
    if (obj) s.download(obj, d_obj, (size_t)n_lp * 8);
    if (iters) s.download(iters, d_it, (size_t)n_lp * 4);
    if (tight) s.download(tight, d_tight, (size_t)n_lp * m * 4);
    s.sync();
    return s.finish();
}

extern "C" int mpc_lp_solve_batch(int32_t device, int64_t n_lp, int32_t m, int32_t n, const double *A, int32_t shared_A, const double *b,
                                  int32_t shared_b, const double *c, int32_t shared_c, const uint8_t *eq, int32_t *status, double *x,
                                  double *obj, int32_t *iters) {
    return lp_batch(device, n_lp, m, n, A, shared_A, b, shared_b, c, shared_c, eq, status, x, obj, iters, nullptr);
}

// ---- the QP of a program at fixed parameter points (qp.hpp) ----------------------------------------------------------------------
// here and in the MIQP call, an output the caller does not take (nullptr) gets an empty buffer: the kernel sees nullptr, nothing is copied back
int mpc::qp_batch(mpc_handle *h, hipStream_t st, int n_cu, const QpProgram &P, int64_t m, const double *theta, int32_t *status, double *x,
                  double *lambda, uint8_t *active, int32_t *iters) {
    const int nc = P.n_c, nt = P.n_t, nx = P.n_x;
    const int ld = odd_at_least(nc + 3);
    const size_t lds = ((size_t)(nc + 1) * ld + nc) * sizeof(double) + (size_t)(ld + 1 + 2 * (nc + 2) + 2) * sizeof(int32_t) + 16;
    if (lds > 160 * 1024) return fail(h, MPC_ERR_INVALID, "the QP tableau (n_c x n_c) does not fit the 160 KiB LDS of one CU");
    if (lds > 48 * 1024) HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_qp_batch), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const size_t sz_x = x ? (size_t)m * nx * sizeof(double) : 0, sz_l = lambda ? (size_t)m * nc * sizeof(double) : 0, sz_a = active ? (size_t)m * nc : 0;
    OneShot s("mpc_qp_solve_batch", st);
    DevBuf &d_th = s.upload(theta, (size_t)m * nt * sizeof(double)), &d_st = s.buf((size_t)m * sizeof(int32_t)), &d_it = s.buf((size_t)m * sizeof(int32_t));
    DevBuf &d_x = s.buf(sz_x), &d_l = s.buf(sz_l), &d_a = s.buf(sz_a), &d_w = s.buf(4);
    s.fill(d_w, 0, 4);
    s.launch([&] {
        const int per_cu = std::max(1, std::min(16, (int)((160 * 1024) / lds)));
        const dim3 g((unsigned)std::min<long long>(m, (long long)n_cu * per_cu)), b(64);
        hipLaunchKernelGGL(k_qp_batch, g, b, lds, st, (long long)m, nc, P.n_eq, nt, nx, ld, P.W, P.UV, P.X0H, P.Gt, d_th.as<double>(), d_st.as<int32_t>(),
                           d_x.as<double>(), d_l.as<double>(), d_a.as<uint8_t>(), d_it.as<int32_t>(), d_w.as<unsigned int>());
    });
    s.download(status, d_st, (size_t)m * sizeof(int32_t));
    if (iters) s.download(iters, d_it, (size_t)m * sizeof(int32_t));
    s.download(x, d_x, sz_x);
    s.download(lambda, d_l, sz_l);
    s.download(active, d_a, sz_a);
    s.sync();
    return s.finish(h);
}

// ---- the MIQP at fixed parameter points: every (point, fixation) pair, pick, winners (qp.hpp) ------------------------------------
extern "C" int mpc_miqp_solve_batch(int32_t device, int32_t n_c, int32_t n_eq, int32_t n_x, int32_t n_t, int32_t n_b, const double *W,
                                    const double *UV, const double *X0, const double *Gt, const double *Q_c, const double *G, const double *K,
                                    int32_t n_check, const double *check, const uint8_t *check_eq, const int32_t *binary_index, int32_t n_rows,
                                    const int32_t *lcp_row, int64_t n_leaves, const double *Y, int64_t m, const double *theta, int32_t *status,
                                    int32_t *leaf, double *obj, double *x, double *lambda, uint8_t *active) {
    const int nxc = n_x - n_b, nz = 1 + n_t + n_b;
    if (n_c < 0 || n_eq < 0 || n_eq > n_c || n_t < 0 || n_b < 0 || nxc < 1 || n_check < 0 || n_rows < n_c || n_leaves < 0 || m < 0)
        return fail(nullptr, MPC_ERR_INVALID, "mpc_miqp_solve_batch: bad sizes");
    if ((n_c && (!W || !UV || !Gt || !lcp_row)) || !X0 || !Q_c || !G || !K || (n_check && (!check || !check_eq)) || (n_b && !binary_index) ||
        (n_leaves && n_b && !Y) || (m && (!status || !leaf || !obj)) || (m && n_t && !theta))
        return fail(nullptr, MPC_ERR_INVALID, "mpc_miqp_solve_batch: missing array");
    // every index the kernels write through is checked here
    std::vector<int32_t> cont;
    {
        std::vector<char> is_bin((size_t)n_x, 0);
        for (int k = 0; k < n_b; ++k) {
            if (binary_index[k] < 0 || binary_index[k] >= n_x || is_bin[binary_index[k]]) return fail(nullptr, MPC_ERR_INVALID, "mpc_miqp_solve_batch: bad binary_index");
            is_bin[binary_index[k]] = 1;
        }
        for (int a = 0; a < n_x; ++a) if (!is_bin[a]) cont.push_back(a);
        for (int i = 0; i < n_c; ++i) if (lcp_row[i] < 0 || lcp_row[i] >= n_rows) return fail(nullptr, MPC_ERR_INVALID, "mpc_miqp_solve_batch: bad lcp_row");
    }
    if (m == 0) return MPC_OK;
    if (n_leaves == 0) {
        for (long long p = 0; p < m; ++p) { status[p] = QP_INFEASIBLE; leaf[p] = -1; obj[p] = NAN; }
        if (x) std::fill(x, x + (size_t)m * n_x, NAN);
        if (lambda) std::fill(lambda, lambda + (size_t)m * n_rows, 0.0);
        if (active) std::fill(active, active + (size_t)m * n_rows, (uint8_t)0);
        return MPC_OK;
    }
    if (int rc = select_device(nullptr, device)) return rc;
    const int ld = odd_at_least(n_c + 3);
    // the k_qp_batch tableau and multipliers, then z and x
    const size_t lds = ((size_t)(n_c + 1) * ld + n_c + nz + nxc) * sizeof(double) + (size_t)(ld + 1 + 2 * (n_c + 2) + 2) * sizeof(int32_t) + 16;
    if (lds > 160 * 1024) return fail(nullptr, MPC_ERR_INVALID, "the QP tableau (n_c x n_c) does not fit the 160 KiB LDS of one CU");
    for (const void *k : {reinterpret_cast<const void *>(k_miqp_pairs), reinterpret_cast<const void *>(k_miqp_winners)})
        if (lds > 48 * 1024) HIP_TRY(nullptr, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // constant blocks in one allocation: W UV X0 Gt Qc G K CK Y theta | ck_eq | cont bin lcp_row
    const size_t nW = (size_t)n_c * n_c, nUV = (size_t)n_c * nz, nX0 = (size_t)nxc * nz, nGt = (size_t)n_c * nxc, nQ = (size_t)nxc * nxc;
    const size_t nG = (size_t)nxc * nz, nK = (size_t)nz * nz, nCK = (size_t)n_check * nz, nY = (size_t)n_leaves * n_b, nTh = (size_t)m * n_t;
    const size_t nd = nW + nUV + nX0 + nGt + nQ + nG + nK + nCK + nY + nTh, ni = (size_t)nxc + n_b + n_c;
    std::vector<double> hd(std::max<size_t>(nd, 1));
    std::vector<int32_t> hi(std::max<size_t>(ni, 1));
    size_t o = 0;
    auto put = [&](const double *src, size_t n) { const size_t at = o; if (n) std::copy(src, src + n, hd.begin() + at); o += n; return at; };
    const size_t oW = put(W, nW), oUV = put(UV, nUV), oX0 = put(X0, nX0), oGt = put(Gt, nGt), oQ = put(Q_c, nQ), oG = put(G, nG), oK = put(K, nK);
    const size_t oCK = put(check, nCK), oY = put(Y, nY), oTh = put(theta, nTh);
    std::copy(cont.begin(), cont.end(), hi.begin());
    if (n_b) std::copy(binary_index, binary_index + n_b, hi.begin() + nxc);
    if (n_c) std::copy(lcp_row, lcp_row + n_c, hi.begin() + nxc + n_b);
    const long long n_pairs = m * n_leaves;
    const size_t sz_x = x ? (size_t)m * n_x * 8 : 0, sz_l = lambda ? (size_t)m * n_rows * 8 : 0, sz_a = active ? (size_t)m * n_rows : 0;
    OneShot s("mpc_miqp_solve_batch", OneShot::OwnStream{});
    DevBuf &d_d = s.upload(hd.data(), hd.size() * 8), &d_i = s.upload(hi.data(), hi.size() * 4), &d_ck = s.upload(check_eq, (size_t)n_check);
    DevBuf &d_ps = s.buf((size_t)n_pairs * 4), &d_po = s.buf((size_t)n_pairs * 8);
    DevBuf &d_st = s.buf((size_t)m * 4), &d_leaf = s.buf((size_t)m * 4), &d_best = s.buf((size_t)m * 8), &d_obj = s.buf((size_t)m * 8), &d_w = s.buf(16);
    DevBuf &d_x = s.buf(sz_x), &d_l = s.buf(sz_l), &d_a = s.buf(sz_a);
    s.fill(d_w, 0, 16);
    if (x) s.fill(d_x, 0xff, sz_x);   // all-ones bytes: a NaN where no pair is optimal
    if (lambda) s.fill(d_l, 0, sz_l);
    if (active) s.fill(d_a, 0, sz_a);
    const double *dd = d_d.as<double>();
    const int32_t *di = d_i.as<int32_t>();
    const MiqpBlocks B{n_c, n_eq, nxc, n_t, n_b, nz, n_check, n_x, n_rows, dd + oW, dd + oUV, dd + oX0, dd + oGt, dd + oQ, dd + oG, dd + oK,
                       dd + oCK, dd + oY, dd + oTh, d_ck.as<uint8_t>(), di, di + nxc, di + nxc + n_b};
    const int n_cu = std::max(cu_count(device), 1), per_cu = waves_per_cu((int)lds);
    unsigned int *work = d_w.as<unsigned int>();
    s.launch([&] {
        hipLaunchKernelGGL(k_miqp_pairs, dim3((unsigned)std::min<long long>(n_pairs, (long long)n_cu * per_cu)), dim3(64), lds, s.st, B, (long long)m,
                           (long long)n_leaves, ld, d_ps.as<int32_t>(), d_po.as<double>(), work);
        hipLaunchKernelGGL(k_miqp_pick, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s.st, (long long)m, (long long)n_leaves, d_ps.as<int32_t>(),
                           d_po.as<double>(), d_st.as<int32_t>(), d_leaf.as<int32_t>(), d_best.as<double>());
        hipLaunchKernelGGL(k_miqp_winners, dim3((unsigned)std::min<long long>(m, (long long)n_cu * per_cu)), dim3(64), lds, s.st, B, (long long)m, ld,
                           d_leaf.as<int32_t>(), d_obj.as<double>(), d_x.as<double>(), d_l.as<double>(), d_a.as<uint8_t>(), work + 2);
    });
    std::vector<double> again((size_t)m);
    s.download(status, d_st, (size_t)m * 4);
    s.download(leaf, d_leaf, (size_t)m * 4);
    s.download(obj, d_best, (size_t)m * 8);
    s.download(x, d_x, sz_x);
    s.download(lambda, d_l, sz_l);
    s.download(active, d_a, sz_a);
    s.download(again.data(), d_obj, (size_t)m * 8);
    s.sync();
    if (int rc = s.finish()) return rc;
    // the winner pass repeats the arithmetic of pass 1: its objective must be the one that won, bit for bit
    for (long long p = 0; p < m; ++p)
        if (leaf[p] >= 0 && std::memcmp(&again[(size_t)p], &obj[p], 8) != 0) return fail(nullptr, MPC_ERR_STATE, "mpc_miqp_solve_batch: the winner pass disagrees with pass 1");
    return MPC_OK;
}
