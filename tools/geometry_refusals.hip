// geometry_refusals.hip -- the argument checking of the merge, overlap, transition, exit, reduce, support, project, backward-exit and forward-cell calls
// (mpc_merge_regions, mpc_merge_pairs, mpc_overlap_pairs, mpc_overlap_split, mpc_transition_boxes, mpc_transition_pairs, mpc_exit_split,
// mpc_reduce_rows, mpc_support_rows, mpc_project_rows, mpc_backward_exits, mpc_forward_cells) as a stand-alone host program for a sanitizer build (DESIGN §3.14,
// §3.19 to §3.25, §3.28):
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/geometry_refusals.hip -o geometry_refusals
// It includes geometry.hip itself and stands in for the pools of mpcombi_hip.hip, which a refusal never reaches: every call below must
// come back MPC_ERR_INVALID with a message before a device is selected (an empty batch: MPC_OK), so the program needs no GPU and
// launches nothing.  The arguments are heap copies of exactly the sizes they promise: a read past them is the sanitizer's to report.
#include "../ppopt_amd/csrc/geometry.hip"

#include <cstdlib>

static std::string g_msg;
namespace mpc {
int fail(mpc_handle *, int code, const std::string &msg) { g_msg = msg; return code; }
size_t dev_size_class(size_t bytes) { return bytes; }
hipError_t dev_pool_take(size_t, void **) { std::abort(); }
void dev_pool_give(void *, size_t) { std::abort(); }
hipError_t host_pool_take(size_t, void **, size_t *, bool) { std::abort(); }
bool host_pool_give(void *) { std::abort(); }
hipError_t pooled_stream(hipStream_t *) { std::abort(); }
void return_stream(hipStream_t) { std::abort(); }
hipError_t pooled_event(hipEvent_t *, bool) { std::abort(); }
void return_event(hipEvent_t, bool) { std::abort(); }
int device_count_cached() { std::abort(); }      // reached only by a call that was not refused
int cu_count(int) { std::abort(); }
}  // namespace mpc

static int n_bad = 0;
static void expect(const char *what, int rc, int want = MPC_ERR_INVALID) {
    const bool ok = rc == want && (want == MPC_OK) == g_msg.empty();
    std::printf("%-44s rc = %d  %s\n", what, rc, g_msg.c_str());
    if (!ok) ++n_bad;
    g_msg.clear();
}

using VD = std::vector<double>;
using VI = std::vector<int32_t>;
using VL = std::vector<int64_t>;

// mpc_merge_regions, mpc_merge_pairs
static void merge_cases() {
    const int nt = 2;
    const VD sq{1, 1, 0, 1, 0, 1, 0, -1, 0, 0, 0, -1};                                                 // [0, 1]^2
    VD ef = sq;
    ef.insert(ef.end(), {1.5, 1, 0, 1, 0, 1, -0.5, -1, 0, 0, 0, -1});                                  // [1/2, 3/2] x [0, 1]
    VD out_xs(4), out_box(8), t_max(1);
    VI status(2), verdict(1);
    std::vector<uint64_t> env_a(MPC_MERGE_WORDS), env_b(MPC_MERGE_WORDS);
    int64_t stats[7];
    float ms = 0.0f;
    struct Args { int n_t; VL off; VD ef, xs, box; VI a, b; double tol; };
    const Args good{nt, {0, 4, 8}, ef, {0.5, 0.5, 1.0, 0.5}, {0, 0, 1, 1, 0.5, 0, 1.5, 1}, {0}, {1}, 1e-8};
    auto regions = [&](const Args &g) {
        return mpc_merge_regions(0, g.n_t, (int64_t)g.off.size() - 1, g.off.data(), g.ef.data(), out_xs.data(), out_box.data(), status.data(), stats, &ms);
    };
    auto pairs = [&](const Args &g, int64_t n_pairs = -2) {
        return mpc_merge_pairs(0, g.n_t, (int64_t)g.off.size() - 1, g.off.data(), g.ef.data(), g.xs.data(), g.box.data(),
                               n_pairs == -2 ? (int64_t)g.a.size() : n_pairs, g.a.data(), g.b.data(), g.tol, env_a.data(), env_b.data(), verdict.data(),
                               t_max.data(), stats, &ms);
    };
    auto with = [&](auto change) { Args g = good; change(g); return g; };
    const double nan = std::nan("");
    VD big;                                                                                            // 257 rows
    for (int r = 0; r < 64; ++r) big.insert(big.end(), sq.begin(), sq.end());
    big.insert(big.end(), sq.begin(), sq.begin() + 3);
    auto one_big = [&](Args &g) { g.off = {0, 257}; g.ef = big; g.xs.resize(2); g.box.resize(4); g.a = {0}; g.b = {0}; };
    expect("merge_regions: n_t = 0", regions(with([](Args &g) { g.n_t = 0; })));
    expect("merge_regions: n_t = 17", regions(with([](Args &g) { g.n_t = 17; })));
    expect("merge_regions: row_off[0] != 0", regions(with([](Args &g) { g.off = {1, 4, 8}; })));
    expect("merge_regions: a region without rows", regions(with([](Args &g) { g.off = {0, 0, 8}; })));
    expect("merge_regions: a region of 257 rows", regions(with(one_big)));
    expect("merge_regions: a non-finite row", regions(with([&](Args &g) { g.ef[4] = nan; })));
    expect("merge_regions: a row that is not unit", regions(with([](Args &g) { g.ef[1] = 2.0; })));
    expect("merge_regions: n_regions < 0", mpc_merge_regions(0, nt, -1, good.off.data(), ef.data(), out_xs.data(), out_box.data(), status.data(), nullptr, nullptr));
    expect("merge_regions: missing row_off", mpc_merge_regions(0, nt, 2, nullptr, ef.data(), out_xs.data(), out_box.data(), status.data(), nullptr, nullptr));
    expect("merge_regions: missing ef_rows", mpc_merge_regions(0, nt, 2, good.off.data(), nullptr, out_xs.data(), out_box.data(), status.data(), nullptr, nullptr));
    expect("merge_regions: missing xs", mpc_merge_regions(0, nt, 2, good.off.data(), ef.data(), nullptr, out_box.data(), status.data(), nullptr, nullptr));
    expect("merge_regions: missing box", mpc_merge_regions(0, nt, 2, good.off.data(), ef.data(), out_xs.data(), nullptr, status.data(), nullptr, nullptr));
    expect("merge_regions: missing status", mpc_merge_regions(0, nt, 2, good.off.data(), ef.data(), out_xs.data(), out_box.data(), nullptr, nullptr, nullptr));
    expect("merge_regions: no regions is MPC_OK without a launch", mpc_merge_regions(0, nt, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), MPC_OK);
    expect("merge_pairs: n_t = 0", pairs(with([](Args &g) { g.n_t = 0; })));
    expect("merge_pairs: n_t = 17", pairs(with([](Args &g) { g.n_t = 17; })));
    expect("merge_pairs: row_off[0] != 0", pairs(with([](Args &g) { g.off = {1, 4, 8}; })));
    expect("merge_pairs: a region without rows", pairs(with([](Args &g) { g.off = {0, 0, 8}; })));
    expect("merge_pairs: a region of 257 rows", pairs(with(one_big)));
    expect("merge_pairs: a non-finite row", pairs(with([](Args &g) { g.ef[12] = INFINITY; })));
    expect("merge_pairs: a row that is not unit", pairs(with([](Args &g) { g.ef[14] = 0.5; })));
    expect("merge_pairs: tol < 0", pairs(with([](Args &g) { g.tol = -1.0; })));
    expect("merge_pairs: tol NaN", pairs(with([&](Args &g) { g.tol = nan; })));
    expect("merge_pairs: tol inf", pairs(with([](Args &g) { g.tol = INFINITY; })));
    expect("merge_pairs: n_pairs < 0", pairs(good, -1));
    expect("merge_pairs: n_pairs = 2^31", pairs(good, 0x80000000ll));
    expect("merge_pairs: region index out of range", pairs(with([](Args &g) { g.b = {2}; })));
    expect("merge_pairs: negative region index", pairs(with([](Args &g) { g.a = {-1}; })));
    expect("merge_pairs: the same region twice", pairs(with([](Args &g) { g.b = {0}; })));
    expect("merge_pairs: xs NaN", pairs(with([&](Args &g) { g.xs[3] = nan; })));
    expect("merge_pairs: xs inf", pairs(with([](Args &g) { g.xs[0] = -INFINITY; })));
    const Args &g = good;
    auto raw = [&](const double *xs, const double *box, const int32_t *a, const int32_t *b, uint64_t *ea, uint64_t *eb, int32_t *v, double *t) {
        return mpc_merge_pairs(0, nt, 2, g.off.data(), g.ef.data(), xs, box, 1, a, b, 1e-8, ea, eb, v, t, nullptr, nullptr);
    };
    expect("merge_pairs: missing xs", raw(nullptr, g.box.data(), g.a.data(), g.b.data(), env_a.data(), env_b.data(), verdict.data(), t_max.data()));
    expect("merge_pairs: missing box", raw(g.xs.data(), nullptr, g.a.data(), g.b.data(), env_a.data(), env_b.data(), verdict.data(), t_max.data()));
    expect("merge_pairs: missing pair_a", raw(g.xs.data(), g.box.data(), nullptr, g.b.data(), env_a.data(), env_b.data(), verdict.data(), t_max.data()));
    expect("merge_pairs: missing pair_b", raw(g.xs.data(), g.box.data(), g.a.data(), nullptr, env_a.data(), env_b.data(), verdict.data(), t_max.data()));
    expect("merge_pairs: missing env_a", raw(g.xs.data(), g.box.data(), g.a.data(), g.b.data(), nullptr, env_b.data(), verdict.data(), t_max.data()));
    expect("merge_pairs: missing env_b", raw(g.xs.data(), g.box.data(), g.a.data(), g.b.data(), env_a.data(), nullptr, verdict.data(), t_max.data()));
    expect("merge_pairs: missing verdict", raw(g.xs.data(), g.box.data(), g.a.data(), g.b.data(), env_a.data(), env_b.data(), nullptr, t_max.data()));
    expect("merge_pairs: missing t_max", raw(g.xs.data(), g.box.data(), g.a.data(), g.b.data(), env_a.data(), env_b.data(), verdict.data(), nullptr));
    expect("merge_pairs: no pairs is MPC_OK without a launch", pairs(with([](Args &a) { a.a.clear(); a.b.clear(); })), MPC_OK);
    expect("merge_pairs: no pairs, no pair arrays", mpc_merge_pairs(0, nt, 2, g.off.data(), g.ef.data(), nullptr, nullptr, 0, nullptr, nullptr, 1e-8, nullptr, nullptr,
                                                                    nullptr, nullptr, nullptr, nullptr), MPC_OK);
}

// mpc_overlap_pairs, mpc_overlap_split
static void overlap_cases() {
    const int nt = 2;
    std::vector<int64_t> off{0, 4, 8};
    std::vector<double> ef{1, 1, 0, 1, 0, 1, 0, -1, 0, 0, 0, -1, 1.5, 1, 0, 1, 0, 1, -0.5, -1, 0, 0, 0, -1};
    std::vector<double> xs{0.5, 0.5, 1.0, 0.5}, cut{0.0, 1.0, 0.0}, out(3);
    std::vector<int32_t> a{0}, b{1}, hc{1}, flag(1);
    std::vector<uint64_t> mask(4);
    std::vector<int64_t> poff{0, 4};
    std::vector<double> pef(ef.begin(), ef.begin() + 12);
    auto pairs = [&](int n_t, const std::vector<int64_t> &o, const std::vector<double> &e, const std::vector<int32_t> &pa,
                     const std::vector<int32_t> &pb, const std::vector<double> &c, double tol) {
        return mpc_overlap_pairs(0, n_t, (int64_t)o.size() - 1, o.data(), e.data(), xs.data(), (int64_t)pa.size(), pa.data(), pb.data(), hc.data(),
                                 c.data(), tol, &out[0], &out[1], &out[2], flag.data(), nullptr, nullptr);
    };
    auto split = [&](const std::vector<int64_t> &po, const std::vector<double> &pe, const std::vector<int32_t> &ip, const std::vector<int32_t> &ic,
                     double tol) {
        return mpc_overlap_split(0, nt, 2, off.data(), ef.data(), (int64_t)po.size() - 1, po.data(), pe.data(), (int64_t)ip.size(), ip.data(),
                                 ic.data(), hc.data(), cut.data(), nullptr, tol, flag.data(), mask.data(), nullptr, nullptr);
    };
    expect("pairs: n_t = 0", pairs(0, off, ef, a, b, cut, 1e-8));
    expect("pairs: n_t = 17", pairs(17, off, ef, a, b, cut, 1e-8));
    expect("pairs: tol < 0", pairs(nt, off, ef, a, b, cut, -1.0));
    expect("pairs: tol NaN", pairs(nt, off, ef, a, b, cut, std::nan("")));
    expect("pairs: region index out of range", pairs(nt, off, ef, a, std::vector<int32_t>{2}, cut, 1e-8));
    expect("pairs: negative region index", pairs(nt, off, ef, std::vector<int32_t>{-1}, b, cut, 1e-8));
    expect("pairs: a region without rows", pairs(nt, std::vector<int64_t>{0, 0, 8}, ef, a, b, cut, 1e-8));
    { std::vector<double> big; for (int r = 0; r < 65; ++r) big.insert(big.end(), ef.begin(), ef.begin() + 12);
      expect("pairs: a region of 260 rows", pairs(nt, std::vector<int64_t>{0, 260}, big, std::vector<int32_t>{}, std::vector<int32_t>{}, cut, 1e-8)); }
    { std::vector<double> v = ef; v[4] = std::nan(""); expect("pairs: a non-finite row", pairs(nt, off, v, a, b, cut, 1e-8)); }
    expect("pairs: a cut row that is not unit", pairs(nt, off, ef, a, b, std::vector<double>{0.0, 2.0, 0.0}, 1e-8));
    expect("split: tol < 0", split(poff, pef, a, b, -1.0));
    expect("split: piece index out of range", split(poff, pef, std::vector<int32_t>{1}, b, 1e-8));
    expect("split: cutter index out of range", split(poff, pef, a, std::vector<int32_t>{2}, 1e-8));
    expect("split: a piece without rows", split(std::vector<int64_t>{0, 0, 4}, pef, std::vector<int32_t>{1}, b, 1e-8));
    { std::vector<double> v = pef; v[0] = INFINITY; expect("split: a non-finite piece row", split(poff, v, a, b, 1e-8)); }
}

// mpc_transition_boxes, mpc_transition_pairs
static void transition_cases() {
    const int nt = 2;
    std::vector<int64_t> off{0, 4, 8};
    VD ef{1, 1, 0, 1, 0, 1, 0, -1, 0, 0, 0, -1, 1.5, 1, 0, 1, 0, 1, -0.5, -1, 0, 0, 0, -1};
    VD Phi{1, 0, 0, 1, 0.5, 0, 0, 0.5}, phi{0, 0, 0.1, 0.1}, xs{0.5, 0.5, 1.0, 0.5}, radius(1), witness(2), box(8);
    VI a{0}, b{1}, status(1), flag(2), none;
    int64_t stats[4];
    float ms = 0.0f;
    struct Args { int n_t; std::vector<int64_t> off; VD ef, Phi, phi, xs; VI a, b; double tol; };
    const Args good{nt, off, ef, Phi, phi, xs, a, b, 1e-8};
    auto pairs = [&](const Args &g, int64_t n_pairs = -2) {
        return mpc_transition_pairs(0, g.n_t, (int64_t)g.off.size() - 1, g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(),
                                    n_pairs == -2 ? (int64_t)g.a.size() : n_pairs, g.a.data(), g.b.data(), 1, g.tol, radius.data(), status.data(),
                                    witness.data(), stats, &ms);
    };
    auto boxes = [&](const Args &g) {
        return mpc_transition_boxes(0, g.n_t, (int64_t)g.off.size() - 1, g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), box.data(),
                                    flag.data(), stats, &ms);
    };
    auto with = [&](auto change) { Args g = good; change(g); return g; };
    const double nan = std::nan("");
    expect("pairs: n_t = 0", pairs(with([](Args &g) { g.n_t = 0; })));
    expect("pairs: n_t = 17", pairs(with([](Args &g) { g.n_t = 17; })));
    expect("pairs: tol < 0", pairs(with([](Args &g) { g.tol = -1.0; })));
    expect("pairs: tol NaN", pairs(with([&](Args &g) { g.tol = nan; })));
    expect("pairs: tol inf", pairs(with([](Args &g) { g.tol = INFINITY; })));
    expect("pairs: n_pairs < 0", pairs(good, -1));
    expect("pairs: n_pairs = 2^31", pairs(good, 0x80000000ll));
    expect("pairs: region index out of range", pairs(with([](Args &g) { g.b = {2}; })));
    expect("pairs: negative region index", pairs(with([](Args &g) { g.a = {-1}; })));
    expect("pairs: a region without rows", pairs(with([](Args &g) { g.off = {0, 0, 8}; })));
    { VD big; for (int r = 0; r < 65; ++r) big.insert(big.end(), ef.begin(), ef.begin() + 12);
      expect("pairs: a region of 260 rows", pairs(with([&](Args &g) { g.off = {0, 260}; g.ef = big; g.a = {0}; g.b = {0}; }))); }
    expect("pairs: a non-finite row", pairs(with([&](Args &g) { g.ef[4] = nan; })));
    expect("pairs: a row that is not unit", pairs(with([](Args &g) { g.ef[1] = 2.0; })));
    expect("pairs: Phi NaN", pairs(with([&](Args &g) { g.Phi[7] = nan; })));
    expect("pairs: Phi inf", pairs(with([](Args &g) { g.Phi[0] = INFINITY; })));
    expect("pairs: phi NaN", pairs(with([&](Args &g) { g.phi[3] = nan; })));
    expect("pairs: xs inf", pairs(with([](Args &g) { g.xs[2] = -INFINITY; })));
    expect("pairs: missing Phi", mpc_transition_pairs(0, nt, 2, off.data(), ef.data(), nullptr, phi.data(), xs.data(), 1, a.data(), b.data(), 1, 1e-8,
                                                      radius.data(), status.data(), witness.data(), nullptr, nullptr));
    expect("pairs: missing xs", mpc_transition_pairs(0, nt, 2, off.data(), ef.data(), Phi.data(), phi.data(), nullptr, 1, a.data(), b.data(), 1, 1e-8,
                                                     radius.data(), status.data(), witness.data(), nullptr, nullptr));
    expect("pairs: missing pair_b", mpc_transition_pairs(0, nt, 2, off.data(), ef.data(), Phi.data(), phi.data(), xs.data(), 1, a.data(), nullptr, 1, 1e-8,
                                                         radius.data(), status.data(), witness.data(), nullptr, nullptr));
    expect("pairs: missing witness", mpc_transition_pairs(0, nt, 2, off.data(), ef.data(), Phi.data(), phi.data(), xs.data(), 1, a.data(), b.data(), 1, 1e-8,
                                                          radius.data(), status.data(), nullptr, nullptr, nullptr));
    expect("pairs: missing row_off", mpc_transition_pairs(0, nt, 2, nullptr, ef.data(), Phi.data(), phi.data(), xs.data(), 1, a.data(), b.data(), 1, 1e-8,
                                                          radius.data(), status.data(), witness.data(), nullptr, nullptr));
    expect("pairs: no pairs is MPC_OK without a launch", pairs(with([&](Args &g) { g.a = none; g.b = none; })), MPC_OK);
    expect("boxes: n_t = 17", boxes(with([](Args &g) { g.n_t = 17; })));
    expect("boxes: a region without rows", boxes(with([](Args &g) { g.off = {0, 0, 8}; })));
    expect("boxes: a non-finite row", boxes(with([](Args &g) { g.ef[0] = INFINITY; })));
    expect("boxes: Phi NaN", boxes(with([&](Args &g) { g.Phi[3] = nan; })));
    expect("boxes: phi inf", boxes(with([](Args &g) { g.phi[0] = INFINITY; })));
    expect("boxes: xs NaN", boxes(with([&](Args &g) { g.xs[3] = nan; })));
    expect("boxes: missing phi", mpc_transition_boxes(0, nt, 2, off.data(), ef.data(), Phi.data(), nullptr, xs.data(), box.data(), flag.data(), nullptr, nullptr));
    expect("boxes: missing image_box", mpc_transition_boxes(0, nt, 2, off.data(), ef.data(), Phi.data(), phi.data(), xs.data(), nullptr, flag.data(), nullptr,
                                                            nullptr));
    expect("boxes: missing flag", mpc_transition_boxes(0, nt, 2, off.data(), ef.data(), Phi.data(), phi.data(), xs.data(), box.data(), nullptr, nullptr, nullptr));
    expect("boxes: no regions is MPC_OK without a launch", mpc_transition_boxes(0, nt, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                                                nullptr, nullptr), MPC_OK);
}

// mpc_exit_split
static void exit_cases() {
    const int nt = 2;
    const VD sq{1, 1, 0, 1, 0, 1, 0, -1, 0, 0, 0, -1};                                                 // [0, 1]^2
    VD ef = sq;
    ef.insert(ef.end(), {1.5, 1, 0, 1, 0, 1, -0.5, -1, 0, 0, 0, -1});                                  // [1/2, 3/2] x [0, 1]
    VI flag(1);
    std::vector<uint64_t> mask(MPC_MERGE_WORDS);
    int64_t stats[5];
    float ms = 0.0f;
    struct Args { int n_t; VL off; VD ef, Phi, phi; VL poff; VD pef; VI p, i, j; VD start; double tol; };
    const Args good{nt, {0, 4, 8}, ef, {1, 0, 0, 1, 0.5, 0, 0, 0.5}, {0, 0, 0.1, 0.1}, {0, 4}, sq, {0}, {0}, {1}, {0.5, 0.5}, 1e-8};
    auto split = [&](const Args &g, int64_t n_items = -2) {
        return mpc_exit_split(0, g.n_t, (int64_t)g.off.size() - 1, g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), (int64_t)g.poff.size() - 1,
                              g.poff.data(), g.pef.data(), n_items == -2 ? (int64_t)g.p.size() : n_items, g.p.data(), g.i.data(), g.j.data(),
                              g.start.data(), g.tol, flag.data(), mask.data(), stats, &ms);
    };
    auto with = [&](auto change) { Args g = good; change(g); return g; };
    const double nan = std::nan("");
    VD big;
    for (int r = 0; r < 65; ++r) big.insert(big.end(), sq.begin(), sq.end());
    expect("n_t = 0", split(with([](Args &g) { g.n_t = 0; })));
    expect("n_t = 17", split(with([](Args &g) { g.n_t = 17; })));
    expect("tol < 0", split(with([](Args &g) { g.tol = -1.0; })));
    expect("tol NaN", split(with([&](Args &g) { g.tol = nan; })));
    expect("tol inf", split(with([](Args &g) { g.tol = INFINITY; })));
    expect("n_items < 0", split(good, -1));
    expect("n_items = 2^31", split(good, 0x80000000ll));
    expect("piece index out of range", split(with([](Args &g) { g.p = {1}; })));
    expect("negative piece index", split(with([](Args &g) { g.p = {-1}; })));
    expect("source index out of range", split(with([](Args &g) { g.i = {2}; })));
    expect("negative source index", split(with([](Args &g) { g.i = {-1}; })));
    expect("target index out of range", split(with([](Args &g) { g.j = {2}; })));
    expect("negative target index", split(with([](Args &g) { g.j = {-3}; })));
    expect("a region without rows", split(with([](Args &g) { g.off = {0, 0, 8}; })));
    expect("a piece without rows", split(with([](Args &g) { g.poff = {0, 0}; })));
    expect("row_off[0] != 0", split(with([](Args &g) { g.off = {1, 4, 8}; })));
    expect("a region of 260 rows", split(with([&](Args &g) { g.off = {0, 260}; g.ef = big; g.Phi.resize(4); g.phi.resize(2); g.j = {0}; })));
    expect("a piece of 260 rows", split(with([&](Args &g) { g.poff = {0, 260}; g.pef = big; })));
    expect("a non-finite region row", split(with([&](Args &g) { g.ef[4] = nan; })));
    expect("a region row that is not unit", split(with([](Args &g) { g.ef[1] = 2.0; })));
    expect("a non-finite piece row", split(with([](Args &g) { g.pef[3] = INFINITY; })));
    expect("a piece row that is not unit", split(with([](Args &g) { g.pef[1] = 0.5; })));
    expect("Phi NaN", split(with([&](Args &g) { g.Phi[7] = nan; })));
    expect("Phi inf", split(with([](Args &g) { g.Phi[0] = INFINITY; })));
    expect("phi NaN", split(with([&](Args &g) { g.phi[3] = nan; })));
    expect("phi inf", split(with([](Args &g) { g.phi[0] = -INFINITY; })));
    expect("start NaN", split(with([&](Args &g) { g.start[1] = nan; })));
    expect("start inf", split(with([](Args &g) { g.start[0] = INFINITY; })));
    const Args &g = good;
    auto raw = [&](const int64_t *off, const double *rows, const double *Phi, const double *phi, const int64_t *poff, const double *pef, const int32_t *p,
                   const int32_t *i, const int32_t *j, int32_t *fl, uint64_t *mk) {
        return mpc_exit_split(0, nt, 2, off, rows, Phi, phi, 1, poff, pef, 1, p, i, j, nullptr, 1e-8, fl, mk, nullptr, nullptr);
    };
    expect("missing row_off", raw(nullptr, g.ef.data(), g.Phi.data(), g.phi.data(), g.poff.data(), g.pef.data(), g.p.data(), g.i.data(), g.j.data(), flag.data(), mask.data()));
    expect("missing ef_rows", raw(g.off.data(), nullptr, g.Phi.data(), g.phi.data(), g.poff.data(), g.pef.data(), g.p.data(), g.i.data(), g.j.data(), flag.data(), mask.data()));
    expect("missing Phi", raw(g.off.data(), g.ef.data(), nullptr, g.phi.data(), g.poff.data(), g.pef.data(), g.p.data(), g.i.data(), g.j.data(), flag.data(), mask.data()));
    expect("missing phi", raw(g.off.data(), g.ef.data(), g.Phi.data(), nullptr, g.poff.data(), g.pef.data(), g.p.data(), g.i.data(), g.j.data(), flag.data(), mask.data()));
    expect("missing piece_off", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), nullptr, g.pef.data(), g.p.data(), g.i.data(), g.j.data(), flag.data(), mask.data()));
    expect("missing piece_rows", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.poff.data(), nullptr, g.p.data(), g.i.data(), g.j.data(), flag.data(), mask.data()));
    expect("missing item_piece", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.poff.data(), g.pef.data(), nullptr, g.i.data(), g.j.data(), flag.data(), mask.data()));
    expect("missing item_source", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.poff.data(), g.pef.data(), g.p.data(), nullptr, g.j.data(), flag.data(), mask.data()));
    expect("missing item_target", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.poff.data(), g.pef.data(), g.p.data(), g.i.data(), nullptr, flag.data(), mask.data()));
    expect("missing flag", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.poff.data(), g.pef.data(), g.p.data(), g.i.data(), g.j.data(), nullptr, mask.data()));
    expect("missing mask", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.poff.data(), g.pef.data(), g.p.data(), g.i.data(), g.j.data(), flag.data(), nullptr));
    expect("no items is MPC_OK without a launch", split(with([](Args &a) { a.p.clear(); a.i.clear(); a.j.clear(); a.start.clear(); })), MPC_OK);
    expect("no items, no pieces, no item arrays", mpc_exit_split(0, nt, 2, g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), 0, nullptr, nullptr, 0, nullptr,
                                                                nullptr, nullptr, nullptr, 1e-8, nullptr, nullptr, nullptr, nullptr), MPC_OK);
}

// mpc_reduce_rows
static void reduce_cases() {
    const int nt = 2;
    const VD sq{1, 1, 0, 1, 0, 1, 0, -1, 0, 0, 0, -1};                                                 // [0, 1]^2
    VD ef = sq;
    ef.insert(ef.end(), {1.5, 1, 0, 1, 0, 1, -0.5, -1, 0, 0, 0, -1});                                  // [1/2, 3/2] x [0, 1]
    VI status(2), wide(2);
    std::vector<uint64_t> kept(2 * MPC_REDUCE_WORDS);
    VD point(4);
    int64_t stats[5];
    float ms = 0.0f;
    struct Args { int n_t; VL off; VD ef, start; double tol; };
    const Args good{nt, {0, 4, 8}, ef, {0.5, 0.5, 1.0, 0.5}, 1e-8};
    auto reduce = [&](const Args &g, int64_t n_poly = -2) {
        return mpc_reduce_rows(0, g.n_t, n_poly == -2 ? (int64_t)g.off.size() - 1 : n_poly, g.off.data(), g.ef.data(), g.start.data(), g.tol, status.data(),
                               wide.data(), kept.data(), point.data(), stats, &ms);
    };
    auto with = [&](auto change) { Args g = good; change(g); return g; };
    const double nan = std::nan("");
    VD big;                                                                                            // 513 rows
    for (int r = 0; r < 128; ++r) big.insert(big.end(), sq.begin(), sq.end());
    big.insert(big.end(), sq.begin(), sq.begin() + 3);
    expect("n_t = 0", reduce(with([](Args &g) { g.n_t = 0; })));
    expect("n_t = 17", reduce(with([](Args &g) { g.n_t = 17; })));
    expect("tol < 0", reduce(with([](Args &g) { g.tol = -1.0; })));
    expect("tol NaN", reduce(with([&](Args &g) { g.tol = nan; })));
    expect("tol inf", reduce(with([](Args &g) { g.tol = INFINITY; })));
    expect("n_poly < 0", reduce(good, -1));
    expect("n_poly = 2^31", reduce(good, 0x80000000ll));
    expect("row_off[0] != 0", reduce(with([](Args &g) { g.off = {1, 4, 8}; })));
    expect("row_off decreases", reduce(with([](Args &g) { g.off = {0, 8, 4}; })));
    expect("a polytope without rows", reduce(with([](Args &g) { g.off = {0, 0, 8}; })));
    expect("a polytope of 513 rows", reduce(with([&](Args &g) { g.off = {0, 513}; g.ef = big; g.start.resize(2); })));
    expect("a non-finite row", reduce(with([&](Args &g) { g.ef[4] = nan; })));
    expect("a row that is not unit", reduce(with([](Args &g) { g.ef[1] = 2.0; })));
    expect("start NaN", reduce(with([&](Args &g) { g.start[1] = nan; })));
    expect("start inf", reduce(with([](Args &g) { g.start[2] = INFINITY; })));
    const Args &g = good;
    auto raw = [&](const int64_t *off, const double *rows, int32_t *st, int32_t *wd, uint64_t *kp) {
        return mpc_reduce_rows(0, nt, 2, off, rows, nullptr, 1e-8, st, wd, kp, nullptr, nullptr, nullptr);
    };
    expect("missing row_off", raw(nullptr, g.ef.data(), status.data(), wide.data(), kept.data()));
    expect("missing ef_rows", raw(g.off.data(), nullptr, status.data(), wide.data(), kept.data()));
    expect("missing status", raw(g.off.data(), g.ef.data(), nullptr, wide.data(), kept.data()));
    expect("missing wide", raw(g.off.data(), g.ef.data(), status.data(), nullptr, kept.data()));
    expect("missing kept", raw(g.off.data(), g.ef.data(), status.data(), wide.data(), nullptr));
    expect("no polytopes is MPC_OK without a launch", reduce(with([](Args &a) { a.off = {0}; a.ef.clear(); a.start.clear(); })), MPC_OK);
    expect("no polytopes, no arrays", mpc_reduce_rows(0, nt, 0, nullptr, nullptr, nullptr, 1e-8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), MPC_OK);
}

// mpc_support_rows
static void support_cases() {
    const int nt = 2;
    const VD sq{1, 1, 0, 1, 0, 1, 0, -1, 0, 0, 0, -1};                                                 // [0, 1]^2
    VD ef = sq;
    ef.insert(ef.end(), {1.5, 1, 0, 1, 0, 1, -0.5, -1, 0, 0, 0, -1});                                  // [1/2, 3/2] x [0, 1]
    VD value(3), arg(6), point(4);
    VI dstat(3), pstat(2), wide(2);
    int64_t stats[7];
    float ms = 0.0f;
    struct Args { int n_t; VL off; VD ef; VL doff; VD dirs, start; double tol; };
    const Args good{nt, {0, 4, 8}, ef, {0, 2, 3}, {1, 0, 0, 0, -1, 2}, {0.5, 0.5, 1.0, 0.5}, 1e-8};
    auto support = [&](const Args &g, int64_t n_poly = -2) {
        return mpc_support_rows(0, g.n_t, n_poly == -2 ? (int64_t)g.off.size() - 1 : n_poly, g.off.data(), g.ef.data(), g.doff.data(), g.dirs.data(),
                                g.start.data(), g.tol, value.data(), arg.data(), dstat.data(), pstat.data(), wide.data(), point.data(), stats, &ms);
    };
    auto with = [&](auto change) { Args g = good; change(g); return g; };
    const double nan = std::nan("");
    VD big;                                                                                            // 513 rows
    for (int r = 0; r < 128; ++r) big.insert(big.end(), sq.begin(), sq.end());
    big.insert(big.end(), sq.begin(), sq.begin() + 3);
    expect("n_t = 0", support(with([](Args &g) { g.n_t = 0; })));
    expect("n_t = 17", support(with([](Args &g) { g.n_t = 17; })));
    expect("tol < 0", support(with([](Args &g) { g.tol = -1.0; })));
    expect("tol NaN", support(with([&](Args &g) { g.tol = nan; })));
    expect("tol inf", support(with([](Args &g) { g.tol = INFINITY; })));
    expect("n_poly < 0", support(good, -1));
    expect("n_poly = 2^31", support(good, 0x80000000ll));
    expect("row_off[0] != 0", support(with([](Args &g) { g.off = {1, 4, 8}; })));
    expect("row_off decreases", support(with([](Args &g) { g.off = {0, 8, 4}; })));
    expect("a polytope without rows", support(with([](Args &g) { g.off = {0, 0, 8}; })));
    expect("a polytope of 513 rows", support(with([&](Args &g) { g.off = {0, 513}; g.ef = big; g.doff = {0, 3}; g.start.resize(2); })));
    expect("a non-finite row", support(with([&](Args &g) { g.ef[4] = nan; })));
    expect("a row that is not unit", support(with([](Args &g) { g.ef[1] = 2.0; })));
    expect("dir_off[0] != 0", support(with([](Args &g) { g.doff = {1, 2, 3}; })));
    expect("dir_off decreases", support(with([](Args &g) { g.doff = {0, 3, 2}; })));
    expect("2^31 directions", support(with([](Args &g) { g.doff = {0, 2, 0x80000000ll}; })));
    expect("a direction NaN", support(with([&](Args &g) { g.dirs[3] = nan; })));
    expect("a direction inf", support(with([](Args &g) { g.dirs[0] = INFINITY; })));
    expect("start NaN", support(with([&](Args &g) { g.start[1] = nan; })));
    expect("start inf", support(with([](Args &g) { g.start[2] = INFINITY; })));
    const Args &g = good;
    auto raw = [&](const int64_t *off, const double *rows, const int64_t *doff, const double *dirs, double *val, int32_t *ds, int32_t *ps, int32_t *wd) {
        return mpc_support_rows(0, nt, 2, off, rows, doff, dirs, nullptr, 1e-8, val, nullptr, ds, ps, wd, nullptr, nullptr, nullptr);
    };
    expect("missing row_off", raw(nullptr, g.ef.data(), g.doff.data(), g.dirs.data(), value.data(), dstat.data(), pstat.data(), wide.data()));
    expect("missing ef_rows", raw(g.off.data(), nullptr, g.doff.data(), g.dirs.data(), value.data(), dstat.data(), pstat.data(), wide.data()));
    expect("missing dir_off", raw(g.off.data(), g.ef.data(), nullptr, g.dirs.data(), value.data(), dstat.data(), pstat.data(), wide.data()));
    expect("missing dirs", raw(g.off.data(), g.ef.data(), g.doff.data(), nullptr, value.data(), dstat.data(), pstat.data(), wide.data()));
    expect("missing value", raw(g.off.data(), g.ef.data(), g.doff.data(), g.dirs.data(), nullptr, dstat.data(), pstat.data(), wide.data()));
    expect("missing dir_status", raw(g.off.data(), g.ef.data(), g.doff.data(), g.dirs.data(), value.data(), nullptr, pstat.data(), wide.data()));
    expect("missing poly_status", raw(g.off.data(), g.ef.data(), g.doff.data(), g.dirs.data(), value.data(), dstat.data(), nullptr, wide.data()));
    expect("missing wide", raw(g.off.data(), g.ef.data(), g.doff.data(), g.dirs.data(), value.data(), dstat.data(), pstat.data(), nullptr));
    expect("no polytopes is MPC_OK without a launch",
           support(with([](Args &a) { a.off = {0}; a.ef.clear(); a.doff = {0}; a.dirs.clear(); a.start.clear(); })), MPC_OK);
    expect("no polytopes, no arrays", mpc_support_rows(0, nt, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 1e-8, nullptr, nullptr, nullptr, nullptr,
                                                       nullptr, nullptr, nullptr, nullptr), MPC_OK);
}

// mpc_project_rows
static void project_cases() {
    const int n = 2;
    const VD sq{1, 1, 0, 1, 0, 1, 0, -1, 0, 0, 0, -1};                                                 // [0, 1]^2
    VD ef = sq;
    ef.insert(ef.end(), {1.5, 1, 0, 1, 0, 1, -0.5, -1, 0, 0, 0, -1});                                  // [1/2, 3/2] x [0, 1]
    const int cap = 8;
    VI status(2), wide(2), n_out(2), peak(2);
    VD out(2 * cap * 2), point(2);
    int64_t stats[9];
    float ms = 0.0f;
    struct Args { int n, n_elim; VL off; VD ef, start; double tol; int out_cap; };
    const Args good{n, 1, {0, 4, 8}, ef, {0.5, 0.5, 1.0, 0.5}, 1e-8, cap};
    auto project = [&](const Args &g, int64_t n_poly = -2) {
        return mpc_project_rows(0, g.n, g.n_elim, n_poly == -2 ? (int64_t)g.off.size() - 1 : n_poly, g.off.data(), g.ef.data(), g.start.data(), g.tol,
                                g.out_cap, out.data(), n_out.data(), status.data(), wide.data(), peak.data(), point.data(), stats, &ms);
    };
    auto with = [&](auto change) { Args g = good; change(g); return g; };
    const double nan = std::nan("");
    VD big;                                                                                            // 513 rows
    for (int r = 0; r < 128; ++r) big.insert(big.end(), sq.begin(), sq.end());
    big.insert(big.end(), sq.begin(), sq.begin() + 3);
    expect("n = 0", project(with([](Args &g) { g.n = 0; })));
    expect("n = 17", project(with([](Args &g) { g.n = 17; })));
    expect("n_elim < 0", project(with([](Args &g) { g.n_elim = -1; })));
    expect("n_elim = n", project(with([](Args &g) { g.n_elim = 2; })));
    expect("tol < 0", project(with([](Args &g) { g.tol = -1.0; })));
    expect("tol NaN", project(with([&](Args &g) { g.tol = nan; })));
    expect("tol inf", project(with([](Args &g) { g.tol = INFINITY; })));
    expect("out_cap = 0", project(with([](Args &g) { g.out_cap = 0; })));
    expect("out_cap = 513", project(with([](Args &g) { g.out_cap = 513; })));
    expect("n_poly < 0", project(good, -1));
    expect("n_poly = 2^31", project(good, 0x80000000ll));
    expect("row_off[0] != 0", project(with([](Args &g) { g.off = {1, 4, 8}; })));
    expect("row_off decreases", project(with([](Args &g) { g.off = {0, 8, 4}; })));
    expect("a polytope without rows", project(with([](Args &g) { g.off = {0, 0, 8}; })));
    expect("a polytope of 513 rows", project(with([&](Args &g) { g.off = {0, 513}; g.ef = big; g.start.resize(2); })));
    expect("a non-finite row", project(with([&](Args &g) { g.ef[4] = nan; })));
    expect("a row that is not unit", project(with([](Args &g) { g.ef[1] = 2.0; })));
    expect("start NaN", project(with([&](Args &g) { g.start[1] = nan; })));
    expect("start inf", project(with([](Args &g) { g.start[2] = INFINITY; })));
    const Args &g = good;
    auto raw = [&](const int64_t *off, const double *rows, double *orows, int32_t *no, int32_t *st, int32_t *wd) {
        return mpc_project_rows(0, n, 1, 2, off, rows, nullptr, 1e-8, cap, orows, no, st, wd, nullptr, nullptr, nullptr, nullptr);
    };
    expect("missing row_off", raw(nullptr, g.ef.data(), out.data(), n_out.data(), status.data(), wide.data()));
    expect("missing ef_rows", raw(g.off.data(), nullptr, out.data(), n_out.data(), status.data(), wide.data()));
    expect("missing out_rows", raw(g.off.data(), g.ef.data(), nullptr, n_out.data(), status.data(), wide.data()));
    expect("missing n_out", raw(g.off.data(), g.ef.data(), out.data(), nullptr, status.data(), wide.data()));
    expect("missing status", raw(g.off.data(), g.ef.data(), out.data(), n_out.data(), nullptr, wide.data()));
    expect("missing wide", raw(g.off.data(), g.ef.data(), out.data(), n_out.data(), status.data(), nullptr));
    expect("no polytopes is MPC_OK without a launch", project(with([](Args &a) { a.off = {0}; a.ef.clear(); a.start.clear(); })), MPC_OK);
    expect("no polytopes, no arrays", mpc_project_rows(0, n, 1, 0, nullptr, nullptr, nullptr, 1e-8, cap, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                        nullptr, nullptr), MPC_OK);
}

// mpc_backward_exits
static void backward_cases() {
    const int nt = 2;
    const VD sq{1, 1, 0, 1, 0, 1, 0, -1, 0, 0, 0, -1};                                                 // [0, 1]^2
    VD ef = sq;
    ef.insert(ef.end(), {1.5, 1, 0, 1, 0, 1, -0.5, -1, 0, 0, 0, -1});                                  // [1/2, 3/2] x [0, 1]
    const int64_t cap_cells = 4, cap_rows = 16;
    int64_t n_cells = -1, stats[6], per_step[4];
    VL out_off(cap_cells + 1);
    VD out_rows(cap_rows * (nt + 1)), out_point(cap_cells * nt);
    VI src(cap_cells), stp(cap_cells), par(cap_cells), wid(cap_cells);
    int32_t status = -1, steps = -1, converged = -1;
    float step_ms[3], ms = 0.0f;
    struct Args { int n_t; VL off; VD ef, Phi, phi, xs; VL poff; VI pidx; VL coff; VD cef; VI csrc; double tol; int max_steps; int64_t max_cells, max_rows; };
    const Args good{nt, {0, 4, 8}, ef, {1, 0, 0, 1, 0.5, 0, 0, 0.5}, {0, 0, 0.1, 0.1}, {0.5, 0.5, 1.0, 0.5}, {0, 1, 2}, {1, 0}, {0, 4}, sq, {0}, 1e-8, 3,
                    cap_cells, cap_rows};
    auto run = [&](const Args &g, int64_t n_cells0 = -2) {
        return mpc_backward_exits(0, g.n_t, (int64_t)g.off.size() - 1, g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), g.poff.data(),
                                  g.pidx.data(), n_cells0 == -2 ? (int64_t)g.csrc.size() : n_cells0, g.coff.data(), g.cef.data(), g.csrc.data(), g.tol,
                                  g.max_steps, g.max_cells, g.max_rows, &n_cells, out_off.data(), out_rows.data(), src.data(), stp.data(), par.data(),
                                  wid.data(), out_point.data(), &status, &steps, &converged, per_step, step_ms, stats, &ms);
    };
    auto with = [&](auto change) { Args g = good; change(g); return g; };
    const double nan = std::nan("");
    VD big;
    for (int r = 0; r < 65; ++r) big.insert(big.end(), sq.begin(), sq.end());
    expect("n_t = 0", run(with([](Args &g) { g.n_t = 0; })));
    expect("n_t = 17", run(with([](Args &g) { g.n_t = 17; })));
    expect("tol < 0", run(with([](Args &g) { g.tol = -1.0; })));
    expect("tol NaN", run(with([&](Args &g) { g.tol = nan; })));
    expect("tol inf", run(with([](Args &g) { g.tol = INFINITY; })));
    expect("max_steps < 0", run(with([](Args &g) { g.max_steps = -1; })));
    expect("max_cells < 0", run(with([](Args &g) { g.max_cells = -1; })));
    expect("max_rows_total < 0", run(with([](Args &g) { g.max_rows = -1; })));
    expect("n_cells0 < 0", run(good, -1));
    expect("n_cells0 = 2^31", run(good, 0x80000000ll));
    expect("a region without rows", run(with([](Args &g) { g.off = {0, 0, 8}; })));
    expect("row_off[0] != 0", run(with([](Args &g) { g.off = {1, 4, 8}; })));
    expect("a region of 260 rows", run(with([&](Args &g) { g.off = {0, 260}; g.ef = big; g.Phi.resize(4); g.phi.resize(2); g.xs.resize(2); g.poff = {0, 0}; })));
    expect("a cell without rows", run(with([](Args &g) { g.coff = {0, 0}; })));
    expect("a cell of 260 rows", run(with([&](Args &g) { g.coff = {0, 260}; g.cef = big; g.max_rows = 512; })));
    expect("cell_off[0] != 0", run(with([](Args &g) { g.coff = {1, 4}; })));
    expect("a non-finite region row", run(with([&](Args &g) { g.ef[4] = nan; })));
    expect("a region row that is not unit", run(with([](Args &g) { g.ef[1] = 2.0; })));
    expect("a non-finite cell row", run(with([](Args &g) { g.cef[3] = INFINITY; })));
    expect("a cell row that is not unit", run(with([](Args &g) { g.cef[1] = 0.5; })));
    expect("Phi NaN", run(with([&](Args &g) { g.Phi[7] = nan; })));
    expect("phi inf", run(with([](Args &g) { g.phi[0] = -INFINITY; })));
    expect("xs NaN", run(with([&](Args &g) { g.xs[1] = nan; })));
    expect("pred_off[0] != 0", run(with([](Args &g) { g.poff = {1, 1, 2}; })));
    expect("pred_off decreases", run(with([](Args &g) { g.poff = {0, 2, 1}; })));
    expect("predecessor index out of range", run(with([](Args &g) { g.pidx = {1, 2}; })));
    expect("negative predecessor index", run(with([](Args &g) { g.pidx = {-1, 0}; })));
    expect("cell source out of range", run(with([](Args &g) { g.csrc = {2}; })));
    expect("negative cell source", run(with([](Args &g) { g.csrc = {-1}; })));
    expect("step 0 above max_cells", run(with([](Args &g) { g.max_cells = 0; })));
    expect("step 0 above max_rows_total", run(with([](Args &g) { g.max_rows = 3; })));
    const Args &g = good;
    auto raw = [&](const int64_t *off, const double *rows, const double *Phi, const double *phi, const double *xs, const int64_t *poff, const int32_t *pidx,
                   const int64_t *coff, const double *cef, const int32_t *csrc, int64_t *n, int64_t *ooff, double *orows, int32_t *osrc, int32_t *st) {
        return mpc_backward_exits(0, nt, 2, off, rows, Phi, phi, xs, poff, pidx, 1, coff, cef, csrc, 1e-8, 3, cap_cells, cap_rows, n, ooff, orows, osrc,
                                  stp.data(), par.data(), wid.data(), nullptr, st, &steps, &converged, nullptr, nullptr, nullptr, nullptr);
    };
    expect("missing row_off", raw(nullptr, g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), g.poff.data(), g.pidx.data(), g.coff.data(), g.cef.data(), g.csrc.data(), &n_cells, out_off.data(), out_rows.data(), src.data(), &status));
    expect("missing ef_rows", raw(g.off.data(), nullptr, g.Phi.data(), g.phi.data(), g.xs.data(), g.poff.data(), g.pidx.data(), g.coff.data(), g.cef.data(), g.csrc.data(), &n_cells, out_off.data(), out_rows.data(), src.data(), &status));
    expect("missing Phi", raw(g.off.data(), g.ef.data(), nullptr, g.phi.data(), g.xs.data(), g.poff.data(), g.pidx.data(), g.coff.data(), g.cef.data(), g.csrc.data(), &n_cells, out_off.data(), out_rows.data(), src.data(), &status));
    expect("missing phi", raw(g.off.data(), g.ef.data(), g.Phi.data(), nullptr, g.xs.data(), g.poff.data(), g.pidx.data(), g.coff.data(), g.cef.data(), g.csrc.data(), &n_cells, out_off.data(), out_rows.data(), src.data(), &status));
    expect("missing xs", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), nullptr, g.poff.data(), g.pidx.data(), g.coff.data(), g.cef.data(), g.csrc.data(), &n_cells, out_off.data(), out_rows.data(), src.data(), &status));
    expect("missing pred_off", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), nullptr, g.pidx.data(), g.coff.data(), g.cef.data(), g.csrc.data(), &n_cells, out_off.data(), out_rows.data(), src.data(), &status));
    expect("missing pred_idx", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), g.poff.data(), nullptr, g.coff.data(), g.cef.data(), g.csrc.data(), &n_cells, out_off.data(), out_rows.data(), src.data(), &status));
    expect("missing cell_off0", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), g.poff.data(), g.pidx.data(), nullptr, g.cef.data(), g.csrc.data(), &n_cells, out_off.data(), out_rows.data(), src.data(), &status));
    expect("missing cell_rows0", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), g.poff.data(), g.pidx.data(), g.coff.data(), nullptr, g.csrc.data(), &n_cells, out_off.data(), out_rows.data(), src.data(), &status));
    expect("missing cell_source0", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), g.poff.data(), g.pidx.data(), g.coff.data(), g.cef.data(), nullptr, &n_cells, out_off.data(), out_rows.data(), src.data(), &status));
    expect("missing n_cells", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), g.poff.data(), g.pidx.data(), g.coff.data(), g.cef.data(), g.csrc.data(), nullptr, out_off.data(), out_rows.data(), src.data(), &status));
    expect("missing status", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), g.poff.data(), g.pidx.data(), g.coff.data(), g.cef.data(), g.csrc.data(), &n_cells, out_off.data(), out_rows.data(), src.data(), nullptr));
    expect("missing cell_off", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), g.poff.data(), g.pidx.data(), g.coff.data(), g.cef.data(), g.csrc.data(), &n_cells, nullptr, out_rows.data(), src.data(), &status));
    expect("missing cell_rows", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), g.poff.data(), g.pidx.data(), g.coff.data(), g.cef.data(), g.csrc.data(), &n_cells, out_off.data(), nullptr, src.data(), &status));
    expect("missing cell_source", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), g.poff.data(), g.pidx.data(), g.coff.data(), g.cef.data(), g.csrc.data(), &n_cells, out_off.data(), out_rows.data(), nullptr, &status));
    // the empty calls: MPC_OK without a launch, step 0 returned
    expect("max_steps = 0 is MPC_OK without a launch", run(with([](Args &a) { a.max_steps = 0; })), MPC_OK);
    if (n_cells != 1 || status != MPC_BACKWARD_MAX_STEPS || steps != 0 || converged != 0 || out_off[1] != 4 || out_rows[11] != sq[11] || src[0] != 0 ||
        par[0] != -1 || per_step[0] != 1) { std::printf("max_steps = 0: step 0 was not returned\n"); ++n_bad; }
    expect("no cells is MPC_OK without a launch", run(with([](Args &a) { a.coff = {0}; a.cef.clear(); a.csrc.clear(); })), MPC_OK);
    if (n_cells != 0 || status != MPC_BACKWARD_CONVERGED || steps != 0 || converged != 1 || out_off[0] != 0) { std::printf("no cells: not converged\n"); ++n_bad; }
    expect("no cells, no cell arrays, no outputs", mpc_backward_exits(0, nt, 2, g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.xs.data(), g.poff.data(),
                                                                 g.pidx.data(), 0, nullptr, nullptr, nullptr, 1e-8, 3, 0, 0, &n_cells, nullptr, nullptr, nullptr,
                                                                 nullptr, nullptr, nullptr, nullptr, &status, &steps, &converged, nullptr, nullptr, nullptr,
                                                                 nullptr), MPC_OK);
}

// mpc_forward_cells
static void forward_cases() {
    const int nt = 2;
    const VD sq{1, 1, 0, 1, 0, 1, 0, -1, 0, 0, 0, -1};                                                 // [0, 1]^2
    VD ef = sq;
    ef.insert(ef.end(), {1.5, 1, 0, 1, 0, 1, -0.5, -1, 0, 0, 0, -1});                                  // [1/2, 3/2] x [0, 1]
    const int64_t cap_cells = 4, cap_rows = 16;
    int64_t n_cells = -1, stats[6], per_step[4];
    VL out_off(cap_cells + 1);
    VD out_rows(cap_rows * (nt + 1)), out_point(cap_cells * nt), out_map(cap_cells * nt * (nt + 1));
    VI reg(cap_cells), stp(cap_cells), par(cap_cells), wid(cap_cells);
    int32_t status = -1, steps = -1;
    float step_ms[3], ms = 0.0f;
    struct Args { int n_t; VL off; VD ef, Phi, phi; VL soff; VI sidx; VL coff; VD cef; VI creg; VD cpt; double tol; int max_steps; int64_t max_cells, max_rows; };
    const Args good{nt, {0, 4, 8}, ef, {1, 0, 0, 1, 0.5, 0, 0, 0.5}, {0, 0, 0.1, 0.1}, {0, 1, 2}, {1, 0}, {0, 4}, sq, {0}, {0.5, 0.5}, 1e-8, 3, cap_cells, cap_rows};
    auto run = [&](const Args &g, int64_t n_cells0 = -2) {
        return mpc_forward_cells(0, g.n_t, (int64_t)g.off.size() - 1, g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(),
                                 n_cells0 == -2 ? (int64_t)g.creg.size() : n_cells0, g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), g.tol,
                                 g.max_steps, g.max_cells, g.max_rows, &n_cells, out_off.data(), out_rows.data(), reg.data(), stp.data(), par.data(),
                                 wid.data(), out_point.data(), out_map.data(), &status, &steps, per_step, step_ms, stats, &ms);
    };
    auto with = [&](auto change) { Args g = good; change(g); return g; };
    const double nan = std::nan("");
    VD big;
    for (int r = 0; r < 65; ++r) big.insert(big.end(), sq.begin(), sq.end());
    expect("n_t = 0", run(with([](Args &g) { g.n_t = 0; })));
    expect("n_t = 17", run(with([](Args &g) { g.n_t = 17; })));
    expect("tol < 0", run(with([](Args &g) { g.tol = -1.0; })));
    expect("tol NaN", run(with([&](Args &g) { g.tol = nan; })));
    expect("tol inf", run(with([](Args &g) { g.tol = INFINITY; })));
    expect("max_steps < 0", run(with([](Args &g) { g.max_steps = -1; })));
    expect("max_cells < 0", run(with([](Args &g) { g.max_cells = -1; })));
    expect("max_rows_total < 0", run(with([](Args &g) { g.max_rows = -1; })));
    expect("n_cells0 < 0", run(good, -1));
    expect("n_cells0 = 2^31", run(good, 0x80000000ll));
    expect("a region without rows", run(with([](Args &g) { g.off = {0, 0, 8}; })));
    expect("row_off[0] != 0", run(with([](Args &g) { g.off = {1, 4, 8}; })));
    expect("a region of 260 rows", run(with([&](Args &g) { g.off = {0, 260}; g.ef = big; g.Phi.resize(4); g.phi.resize(2); g.soff = {0, 0}; })));
    expect("a cell without rows", run(with([](Args &g) { g.coff = {0, 0}; })));
    expect("a cell of 260 rows", run(with([&](Args &g) { g.coff = {0, 260}; g.cef = big; g.max_rows = 512; })));
    expect("cell_off[0] != 0", run(with([](Args &g) { g.coff = {1, 4}; })));
    expect("a non-finite region row", run(with([&](Args &g) { g.ef[4] = nan; })));
    expect("a region row that is not unit", run(with([](Args &g) { g.ef[1] = 2.0; })));
    expect("a non-finite cell row", run(with([](Args &g) { g.cef[3] = INFINITY; })));
    expect("a cell row that is not unit", run(with([](Args &g) { g.cef[1] = 0.5; })));
    expect("Phi NaN", run(with([&](Args &g) { g.Phi[7] = nan; })));
    expect("phi inf", run(with([](Args &g) { g.phi[0] = -INFINITY; })));
    expect("cell point NaN", run(with([&](Args &g) { g.cpt[1] = nan; })));
    expect("succ_off[0] != 0", run(with([](Args &g) { g.soff = {1, 1, 2}; })));
    expect("succ_off decreases", run(with([](Args &g) { g.soff = {0, 2, 1}; })));
    expect("successor index out of range", run(with([](Args &g) { g.sidx = {1, 2}; })));
    expect("negative successor index", run(with([](Args &g) { g.sidx = {-1, 0}; })));
    expect("cell region out of range", run(with([](Args &g) { g.creg = {2}; })));
    expect("negative cell region", run(with([](Args &g) { g.creg = {-1}; })));
    expect("step 0 above max_cells", run(with([](Args &g) { g.max_cells = 0; })));
    expect("step 0 above max_rows_total", run(with([](Args &g) { g.max_rows = 3; })));
    const Args &g = good;
    auto raw = [&](const int64_t *off, const double *rows, const double *Phi, const double *phi, const int64_t *soff, const int32_t *sidx, const int64_t *coff,
                   const double *cef, const int32_t *creg, const double *cpt, int64_t *n, int64_t *ooff, double *orows, int32_t *oreg, double *opt, double *omap,
                   int32_t *st) {
        return mpc_forward_cells(0, nt, 2, off, rows, Phi, phi, soff, sidx, 1, coff, cef, creg, cpt, 1e-8, 3, cap_cells, cap_rows, n, ooff, orows, oreg,
                                 stp.data(), par.data(), wid.data(), opt, omap, st, &steps, nullptr, nullptr, nullptr, nullptr);
    };
    expect("missing row_off", raw(nullptr, g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), &n_cells, out_off.data(), out_rows.data(), reg.data(), out_point.data(), out_map.data(), &status));
    expect("missing ef_rows", raw(g.off.data(), nullptr, g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), &n_cells, out_off.data(), out_rows.data(), reg.data(), out_point.data(), out_map.data(), &status));
    expect("missing Phi", raw(g.off.data(), g.ef.data(), nullptr, g.phi.data(), g.soff.data(), g.sidx.data(), g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), &n_cells, out_off.data(), out_rows.data(), reg.data(), out_point.data(), out_map.data(), &status));
    expect("missing phi", raw(g.off.data(), g.ef.data(), g.Phi.data(), nullptr, g.soff.data(), g.sidx.data(), g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), &n_cells, out_off.data(), out_rows.data(), reg.data(), out_point.data(), out_map.data(), &status));
    expect("missing succ_off", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), nullptr, g.sidx.data(), g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), &n_cells, out_off.data(), out_rows.data(), reg.data(), out_point.data(), out_map.data(), &status));
    expect("missing succ_idx", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), nullptr, g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), &n_cells, out_off.data(), out_rows.data(), reg.data(), out_point.data(), out_map.data(), &status));
    expect("missing cell_off0", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), nullptr, g.cef.data(), g.creg.data(), g.cpt.data(), &n_cells, out_off.data(), out_rows.data(), reg.data(), out_point.data(), out_map.data(), &status));
    expect("missing cell_rows0", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), g.coff.data(), nullptr, g.creg.data(), g.cpt.data(), &n_cells, out_off.data(), out_rows.data(), reg.data(), out_point.data(), out_map.data(), &status));
    expect("missing cell_region0", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), g.coff.data(), g.cef.data(), nullptr, g.cpt.data(), &n_cells, out_off.data(), out_rows.data(), reg.data(), out_point.data(), out_map.data(), &status));
    expect("missing cell_point0", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), g.coff.data(), g.cef.data(), g.creg.data(), nullptr, &n_cells, out_off.data(), out_rows.data(), reg.data(), out_point.data(), out_map.data(), &status));
    expect("missing n_cells", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), nullptr, out_off.data(), out_rows.data(), reg.data(), out_point.data(), out_map.data(), &status));
    expect("missing status", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), &n_cells, out_off.data(), out_rows.data(), reg.data(), out_point.data(), out_map.data(), nullptr));
    expect("missing cell_off", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), &n_cells, nullptr, out_rows.data(), reg.data(), out_point.data(), out_map.data(), &status));
    expect("missing cell_rows", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), &n_cells, out_off.data(), nullptr, reg.data(), out_point.data(), out_map.data(), &status));
    expect("missing cell_region", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), &n_cells, out_off.data(), out_rows.data(), nullptr, out_point.data(), out_map.data(), &status));
    expect("missing cell_point", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), &n_cells, out_off.data(), out_rows.data(), reg.data(), nullptr, out_map.data(), &status));
    expect("missing cell_map", raw(g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), g.coff.data(), g.cef.data(), g.creg.data(), g.cpt.data(), &n_cells, out_off.data(), out_rows.data(), reg.data(), out_point.data(), nullptr, &status));
    // the empty calls: MPC_OK without a launch, step 0 returned with the identity maps
    expect("max_steps = 0 is MPC_OK without a launch", run(with([](Args &a) { a.max_steps = 0; })), MPC_OK);
    if (n_cells != 1 || status != MPC_FORWARD_DONE || steps != 0 || out_off[1] != 4 || out_rows[11] != sq[11] || reg[0] != 0 || par[0] != -1 ||
        per_step[0] != 1 || out_point[0] != 0.5 || out_map[0] != 1.0 || out_map[1] != 0.0 || out_map[2] != 0.0 || out_map[4] != 1.0) {
        std::printf("max_steps = 0: step 0 was not returned\n"); ++n_bad;
    }
    expect("no cells is MPC_OK without a launch", run(with([](Args &a) { a.coff = {0}; a.cef.clear(); a.creg.clear(); a.cpt.clear(); })), MPC_OK);
    if (n_cells != 0 || status != MPC_FORWARD_EMPTY || steps != 0 || out_off[0] != 0) { std::printf("no cells: not EMPTY\n"); ++n_bad; }
    expect("no cells, no cell arrays, no outputs", mpc_forward_cells(0, nt, 2, g.off.data(), g.ef.data(), g.Phi.data(), g.phi.data(), g.soff.data(), g.sidx.data(), 0,
                                                                 nullptr, nullptr, nullptr, nullptr, 1e-8, 3, 0, 0, &n_cells, nullptr, nullptr, nullptr, nullptr,
                                                                 nullptr, nullptr, nullptr, nullptr, &status, &steps, nullptr, nullptr, nullptr, nullptr), MPC_OK);
}

int main() {
    merge_cases();
    overlap_cases();
    transition_cases();
    exit_cases();
    reduce_cases();
    support_cases();
    project_cases();
    backward_cases();
    forward_cases();
    std::printf("%d unexpected\n", n_bad);
    return n_bad ? 1 : 0;
}
