// Host side of one level of the enumeration: ONE launch site per templated kernel family of kernels.hpp / kernels2.hpp.  The forms of a level in
// mpcombi_hip.hip compute grids and arguments and call these; a launcher maps the handle's selector (fast_t, fast_r, fast_x, mask width) to the
// instantiation, fixes the block size the kernel is written for, and launches.  The caller checks hipGetLastError() where it always did.  The
// instantiations named here are the library's set: a selector without a kernel of its own takes the widest form, as before.  (batch_level.hip
// launches its m_* wrappers -- other templates, K <= 8, an LDS attribute call before each -- with its own switches.)  Host code only.
#pragma once
#include <type_traits>

#include "batch_level.hpp"

namespace mpc {

template <int V> using int_c = std::integral_constant<int, V>;

// fast_t / fast_r -> (parameter width NT, LP slots per wavefront SL) of k_theta2 / k_region2
template <class F> static void with_nt_slots(int fast, F &&f) {
    switch (fast) {
        case 0: f(int_c<4>{}, int_c<1>{}); break;
        case 1: f(int_c<4>{}, int_c<2>{}); break;
        case 2: f(int_c<8>{}, int_c<1>{}); break;
        case 3: f(int_c<8>{}, int_c<2>{}); break;
        case 4: f(int_c<10>{}, int_c<1>{}); break;
        default: f(int_c<10>{}, int_c<2>{}); break;
    }
}
static inline int region2_nt(int fast_r) { return fast_r <= 1 ? 4 : (fast_r <= 3 ? 8 : 10); }   // NT of with_nt_slots (fast_r >= 0)
template <class F> static void with_x_slots(int fast_x, F &&f) { if (fast_x & 1) f(int_c<2>{}); else f(int_c<1>{}); }   // LP slots of k_xq / k_x1
template <class F> static void with_mask_words(int mw, F &&f) { if (mw == 2) f(int_c<2>{}); else f(int_c<4>{}); }      // words of an active-set mask

// k_kkt_thread<K, NT, SP>: K = kd inequality rows (1..10), NT from fast_t, SP = BATCH_KKT_SPREAD lanes per candidate if `spread` (the caller's
// decision, and its grid; instantiated for K <= BATCH_KKT_SPREAD_KMAX only), else 1
static void launch_kkt_thread(int kd, int fast_t, bool spread, dim3 g, hipStream_t st, const DevProblem *pf, const int32_t *cands, long long n, uint8_t *code, double *L,
                              uint8_t *status, const ThetaArgs &ta, LevelCounters *ctr) {
    auto rows = [&](auto K) {
        constexpr int k_ = decltype(K)::value;
        auto go = [&](auto NT, auto SP) { hipLaunchKernelGGL((k_kkt_thread<k_, decltype(NT)::value, decltype(SP)::value>), g, dim3(256), 0, st, pf, cands, n, code, L, status, ta, ctr); };
        auto lanes = [&](auto NT) {
            if constexpr (k_ <= BATCH_KKT_SPREAD_KMAX) { if (spread) { go(NT, int_c<BATCH_KKT_SPREAD>{}); return; } }
            go(NT, int_c<1>{});
        };
        if (fast_t >= 4) lanes(int_c<10>{}); else if (fast_t >= 2) lanes(int_c<8>{}); else lanes(int_c<4>{});
    };
    switch (kd) {
        case 1: rows(int_c<1>{}); break; case 2: rows(int_c<2>{}); break; case 3: rows(int_c<3>{}); break; case 4: rows(int_c<4>{}); break; case 5: rows(int_c<5>{}); break;
        case 6: rows(int_c<6>{}); break; case 7: rows(int_c<7>{}); break; case 8: rows(int_c<8>{}); break; case 9: rows(int_c<9>{}); break; case 10: rows(int_c<10>{}); break;
    }
}
static void launch_theta2(int fast_t, dim3 g, size_t lds, hipStream_t st, const DevProblem *pf, const int32_t *cands, long long n, int k, uint8_t *status, LevelCounters *ctr,
                          const uint8_t *kkcode, const double *Lin, const ThetaArgs &ta, const int32_t *list) {
    with_nt_slots(fast_t, [&](auto NT, auto SL) { hipLaunchKernelGGL((k_theta2<decltype(NT)::value, decltype(SL)::value>), g, dim3(64), lds, st, pf, cands, n, k, status, ctr, kkcode, Lin, ta, list); });
}
// box: nullptr, or the parameter box behind the region2_nt(fast_r)-wide vertex block of ThetaArgs::tvp
static void launch_region2(int fast_r, dim3 g, size_t lds, hipStream_t st, const DevProblem *pr, const int32_t *cands, int k, const int32_t *opt_list, int n_opt, uint8_t *status,
                           double *head_d, int32_t *head_i, int fd, int fi, double *epool, LevelCounters *ctr, const uint8_t *kkcode, const double *Lin, int W, uint8_t *kept_g,
                           int ldk, unsigned int *done_g, const double *box, const RegionStream &rs) {
    with_nt_slots(fast_r, [&](auto NT, auto SL) {
        hipLaunchKernelGGL((k_region2<decltype(NT)::value, decltype(SL)::value>), g, dim3(64), lds, st, pr, cands, k, opt_list, n_opt, status, head_d, head_i, fd, fi, epool, ctr,
                           kkcode, Lin, W, kept_g, ldk, done_g, box, rs);
    });
}
// fast_x: bit 0 = two LP slots per wavefront, fast_x >= 2 = 32 dictionary columns instead of 16
static void launch_x2(int fast_x, dim3 g, hipStream_t st, const DevProblem *pf, const int32_t *cands, int k, const int32_t *list, int n_list, uint8_t *status, LevelCounters *ctr,
                      const DictCache &dc) {
    auto go = [&](auto NXC, auto SL) { hipLaunchKernelGGL((k_x2<decltype(NXC)::value, decltype(SL)::value>), g, dim3(64), 0, st, pf, cands, k, list, n_list, status, ctr, dc); };
    switch (fast_x) {
        case 0: go(int_c<16>{}, int_c<1>{}); break;
        case 1: go(int_c<16>{}, int_c<2>{}); break;
        case 2: go(int_c<32>{}, int_c<1>{}); break;
        default: go(int_c<32>{}, int_c<2>{}); break;
    }
}
static void launch_xq(int fast_x, dim3 g, hipStream_t st, const DevProblem *pf, const int32_t *cands, int k, const int32_t *list, int n_list, uint8_t *status, LevelCounters *ctr,
                      const DictCache &dc, int nxc) {
    with_x_slots(fast_x, [&](auto SL) { hipLaunchKernelGGL((k_xq<decltype(SL)::value>), g, dim3(64), 0, st, pf, cands, k, list, n_list, status, ctr, dc, nxc); });
}
static void launch_x1(int fast_x, dim3 g, hipStream_t st, const DevProblem *pf, const int32_t *x1_list, const int32_t *x1_n, LevelCounters *ctr, const DictCache &dc, int nxc,
                      const int32_t *plan_slot, const int32_t *plan_step) {
    with_x_slots(fast_x, [&](auto SL) { hipLaunchKernelGGL((k_x1<decltype(SL)::value>), g, dim3(64), 0, st, pf, x1_list, x1_n, ctr, dc, nxc, plan_slot, plan_step); });
}
// ---- the kernels that walk active-set masks of mw words ---------------------------------------------------------------------------------------
static void launch_pruned_append(int mw, dim3 g, hipStream_t st, const int32_t *cands, long long n, int k, const uint8_t *status, unsigned long long *out, LevelCounters *ctr, int keep_lowdim) {
    with_mask_words(mw, [&](auto MW) { hipLaunchKernelGGL((k_pruned_append<decltype(MW)::value>), g, dim3(256), 0, st, cands, n, k, status, out, ctr, keep_lowdim); });
}
static void launch_children_count(int mw, dim3 g, hipStream_t st, const DevProblem &P, const int32_t *cands, long long n, int k, const uint8_t *status, const unsigned long long *pruned,
                                  long long n_pruned, unsigned long long *childmask, int32_t *count, int keep_lowdim) {
    with_mask_words(mw, [&](auto MW) { hipLaunchKernelGGL((k_children_count<decltype(MW)::value>), g, dim3(64), 0, st, P, cands, n, k, status, pruned, n_pruned, childmask, count, keep_lowdim); });
}
static void launch_children_count_b(int mw, dim3 g, hipStream_t st, const DevProblem &P, const int32_t *cands, long long n, int k, const uint8_t *status, const unsigned long long *bucketed,
                                    const int32_t *head, unsigned long long *childmask, int32_t *count, int keep_lowdim) {
    with_mask_words(mw, [&](auto MW) { hipLaunchKernelGGL((k_children_count_b<decltype(MW)::value>), g, dim3(64), 0, st, P, cands, n, k, status, bucketed, head, childmask, count, keep_lowdim); });
}
static void launch_pruned_bucket_count(int mw, dim3 g, hipStream_t st, const unsigned long long *pruned, long long n_pruned, int ne, int32_t *head) {
    with_mask_words(mw, [&](auto MW) { hipLaunchKernelGGL((k_pruned_bucket_count<decltype(MW)::value>), g, dim3(256), 0, st, pruned, n_pruned, ne, head); });
}
static void launch_pruned_bucket_scatter(int mw, dim3 g, hipStream_t st, const unsigned long long *pruned, long long n_pruned, int ne, int32_t *head, unsigned long long *out) {
    with_mask_words(mw, [&](auto MW) { hipLaunchKernelGGL((k_pruned_bucket_scatter<decltype(MW)::value>), g, dim3(256), 0, st, pruned, n_pruned, ne, head, out); });
}
// (one workgroup of 1,024 threads: the single-block end of a small level)
static void launch_small_end(int mw, hipStream_t st, const int32_t *cands, int n, int k, const uint8_t *status, unsigned long long *pruned_out, LevelCounters *ctr, int keep_lowdim,
                             int32_t *n_retry, int32_t *n_late, const unsigned int *pub_src2, int pub_n2, unsigned int *pub_dst) {
    with_mask_words(mw, [&](auto MW) {
        hipLaunchKernelGGL((k_small_end<decltype(MW)::value>), dim3(1), dim3(1024), 0, st, cands, n, k, status, pruned_out, ctr, keep_lowdim, n_retry, n_late, pub_src2, pub_n2, pub_dst);
    });
}

}  // namespace mpc
