// exit_refusals.hip -- the argument checking of mpc_exit_split as a stand-alone host program for a sanitizer build:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/exit_refusals.hip -o exit_refusals
// It includes geometry.hip itself and stands in for the pools of mpcombi_hip.hip, which a refusal never reaches: every call below must
// come back MPC_ERR_INVALID with a message before a device is selected (the empty item list: MPC_OK), so the program needs no GPU and
// launches nothing.
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

int main() {
    // heap copies of exactly the sizes the arguments promise: a read past them is the sanitizer's to report
    const int nt = 2;
    using VD = std::vector<double>;
    using VI = std::vector<int32_t>;
    using VL = std::vector<int64_t>;
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
    std::printf("%d unexpected\n", n_bad);
    return n_bad ? 1 : 0;
}
