// transition_refusals.hip -- the argument checking of mpc_transition_boxes / mpc_transition_pairs as a stand-alone host program for a
// sanitizer build:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/transition_refusals.hip -o transition_refusals
// It includes geometry.hip itself and stands in for the pools of mpcombi_hip.hip, which a refusal never reaches: every call below must
// come back MPC_ERR_INVALID with a message before a device is selected (the empty pair list: MPC_OK), so the program needs no GPU and
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
    std::printf("%d unexpected\n", n_bad);
    return n_bad ? 1 : 0;
}
