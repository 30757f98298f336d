// box_pairs_refusals.hip -- the argument checking of the candidate sweep and the row screen (mpc_box_pairs, mpc_pair_screen) as a
// stand-alone host program for a sanitizer build, in the manner of tools/geometry_refusals.hip:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/box_pairs_refusals.hip -o box_pairs_refusals
// It includes geometry.hip itself and stands in for the pools of mpcombi_hip.hip, which a refusal never reaches: every call below must
// come back MPC_ERR_INVALID with a message before a device is selected, or MPC_OK without a launch (a family without a usable box, an
// empty row range, no candidates), so the program needs no GPU.  The arguments are heap copies of exactly the sizes they promise: a
// read past them is the sanitizer's to report.
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
int device_count_cached() { std::abort(); }      // reached only by a call that was neither refused nor empty
int cu_count(int) { std::abort(); }
}  // namespace mpc

static int n_bad = 0;
static void expect(const char *what, int rc, int want = MPC_ERR_INVALID) {
    const bool ok = rc == want && (want == MPC_OK) == g_msg.empty();
    std::printf("%-52s rc = %d  %s\n", what, rc, g_msg.c_str());
    if (!ok) ++n_bad;
    g_msg.clear();
}

using VD = std::vector<double>;
using VL = std::vector<int64_t>;
using VB = std::vector<uint8_t>;

static void box_pair_cases() {
    struct Args { int n_t, mode; VD box_a; VB use_a; VD box_b; VB use_b; double margin; int64_t i0, i1, cap; bool b_given, outputs; };
    // three boxes in 2-D, two in family b
    const Args good{2, MPC_BOX_CROSS, {0, 0, 1, 1, 0.5, 0.5, 2, 2, 3, 3, 4, 4}, {1, 1, 1}, {0, 0, 1, 1, 5, 5, 6, 6}, {1, 1}, 1e-8, 0, 3, 8, true, true};
    VL pa(8), pb(8), rc(3);
    int64_t total = -1, stats[3];
    float ms = 0.0f;
    auto run = [&](const Args &g) {
        const int64_t n_a = (int64_t)g.use_a.size(), n_b = g.b_given ? (int64_t)g.use_b.size() : 0;
        return mpc_box_pairs(0, g.n_t, g.mode, n_a, g.box_a.data(), g.use_a.data(), n_b, g.b_given ? g.box_b.data() : nullptr,
                             g.b_given ? g.use_b.data() : nullptr, g.margin, g.i0, g.i1, g.cap, g.outputs ? pa.data() : nullptr,
                             g.outputs ? pb.data() : nullptr, rc.data(), &total, stats, &ms);
    };
    auto with = [&](auto change) { Args g = good; change(g); return g; };
    expect("box_pairs: n_t = 0", run(with([](Args &g) { g.n_t = 0; })));
    expect("box_pairs: n_t = 17", run(with([](Args &g) { g.n_t = 17; })));
    expect("box_pairs: an unknown mode", run(with([](Args &g) { g.mode = 2; })));
    expect("box_pairs: family a has no box", run(with([](Args &g) { g.use_a.clear(); g.box_a.clear(); g.i1 = 0; })));
    expect("box_pairs: family b has no box", run(with([](Args &g) { g.use_b.clear(); g.box_b.clear(); })));
    expect("box_pairs: CROSS without family b", run(with([](Args &g) { g.b_given = false; })));
    expect("box_pairs: UPPER with another family", run(with([](Args &g) { g.mode = MPC_BOX_UPPER; })));
    expect("box_pairs: i0 < 0", run(with([](Args &g) { g.i0 = -1; })));
    expect("box_pairs: i1 > n_a", run(with([](Args &g) { g.i1 = 4; })));
    expect("box_pairs: i1 < i0", run(with([](Args &g) { g.i0 = 2; g.i1 = 1; })));
    expect("box_pairs: cap < 0", run(with([](Args &g) { g.cap = -1; })));
    expect("box_pairs: cap > 0 without pair arrays", run(with([](Args &g) { g.outputs = false; })));
    expect("box_pairs: margin NaN", run(with([](Args &g) { g.margin = std::nan(""); })));
    expect("box_pairs: margin +inf", run(with([](Args &g) { g.margin = INFINITY; })));
    expect("box_pairs: no total", mpc_box_pairs(0, 2, MPC_BOX_CROSS, 3, good.box_a.data(), good.use_a.data(), 2, good.box_b.data(), good.use_b.data(), 1e-8, 0, 3,
                                                0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    expect("box_pairs: no usable_a", mpc_box_pairs(0, 2, MPC_BOX_UPPER, 3, good.box_a.data(), nullptr, 0, nullptr, nullptr, 1e-8, 0, 3, 0, nullptr, nullptr,
                                                   nullptr, &total, nullptr, nullptr));
    // the zero-pair paths: MPC_OK, total 0, the row counts cleared, no launch
    auto zero = [&](const char *what, const Args &g) {
        total = -1;
        std::fill(rc.begin(), rc.end(), (int64_t)-1);
        expect(what, run(g), MPC_OK);
        const int64_t rows = g.i1 - g.i0;
        bool ok = total == 0 && stats[0] == 0 && stats[1] == 0 && stats[2] == 0 && ms == 0.0f;
        for (int64_t r = 0; r < rows; ++r) ok = ok && rc[r] == 0;
        if (!ok) { std::printf("%s: not an empty result\n", what); ++n_bad; }
    };
    zero("box_pairs: family a without a usable box", with([](Args &g) { g.use_a = {0, 0, 0}; }));
    zero("box_pairs: family b without a usable box", with([](Args &g) { g.use_b = {0, 0}; }));
    zero("box_pairs: an empty row range", with([](Args &g) { g.i0 = g.i1 = 2; }));
    zero("box_pairs: the range holds no usable box", with([](Args &g) { g.use_a = {1, 0, 1}; g.i0 = 1; g.i1 = 2; }));
    zero("box_pairs: UPPER with one usable box", with([](Args &g) { g.mode = MPC_BOX_UPPER; g.b_given = false; g.use_a = {0, 1, 0}; }));
    zero("box_pairs: UPPER, the last row alone", with([](Args &g) { g.mode = MPC_BOX_UPPER; g.b_given = false; g.i0 = 2; g.i1 = 3; }));
    zero("box_pairs: count-only, nothing usable", with([](Args &g) { g.use_a = {0, 0, 0}; g.cap = 0; g.outputs = false; }));
}

static void pair_screen_cases() {
    struct Args { int n_t; VL off; VD ef; VL a, b; VD box_a, box_b; int sides; };
    const VD sq{1, 1, 0, 1, 0, 1, 0, -1, 0, 0, 0, -1};      // [0, 1]^2
    VD ef = sq;
    ef.insert(ef.end(), sq.begin(), sq.end());
    const Args good{2, {0, 4, 8}, ef, {0, 1}, {1, 0}, {0, 0, 1, 1, 0, 0, 1, 1}, {0, 0, 1, 1, 0, 0, 1, 1}, 3};
    std::vector<uint8_t> keep(2);
    int64_t stats[3];
    float ms = 0.0f;
    auto run = [&](const Args &g, int64_t n_pairs = -2, bool with_a = true, bool with_b = true) {
        return mpc_pair_screen(0, g.n_t, (int64_t)g.off.size() - 1, g.off.data(), g.ef.data(), n_pairs == -2 ? (int64_t)g.a.size() : n_pairs, g.a.data(),
                               g.b.data(), with_a ? g.box_a.data() : nullptr, with_b ? g.box_b.data() : nullptr, g.sides, keep.data(), stats, &ms);
    };
    auto with = [&](auto change) { Args g = good; change(g); return g; };
    expect("pair_screen: n_t = 17", run(with([](Args &g) { g.n_t = 17; })));
    expect("pair_screen: a region without rows", run(with([](Args &g) { g.off = {0, 0, 8}; })));
    expect("pair_screen: a row that is not unit", run(with([](Args &g) { g.ef[1] = 2.0; })));
    expect("pair_screen: n_pairs < 0", run(good, -1));
    expect("pair_screen: sides = 0", run(with([](Args &g) { g.sides = 0; })));
    expect("pair_screen: sides = 4", run(with([](Args &g) { g.sides = 4; })));
    expect("pair_screen: side A without its boxes", run(good, -2, false, true));
    expect("pair_screen: side B without its boxes", run(good, -2, true, false));
    expect("pair_screen: pair_a out of range", run(with([](Args &g) { g.a = {0, 2}; })));
    expect("pair_screen: pair_b negative", run(with([](Args &g) { g.b = {-1, 0}; })));
    expect("pair_screen: no keep array", mpc_pair_screen(0, 2, 2, good.off.data(), good.ef.data(), 2, good.a.data(), good.b.data(), good.box_a.data(),
                                                         good.box_b.data(), 3, nullptr, nullptr, nullptr));
    expect("pair_screen: no candidates is MPC_OK", run(good, 0), MPC_OK);
    expect("pair_screen: no candidates, no arrays", mpc_pair_screen(0, 2, 2, good.off.data(), good.ef.data(), 0, nullptr, nullptr, nullptr, nullptr, 1, nullptr,
                                                                    nullptr, nullptr), MPC_OK);
}

int main() {
    box_pair_cases();
    pair_screen_cases();
    std::printf("%d unexpected\n", n_bad);
    return n_bad ? 1 : 0;
}
