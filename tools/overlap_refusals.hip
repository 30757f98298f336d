// overlap_refusals.hip -- the argument checking of mpc_overlap_pairs / mpc_overlap_split as a stand-alone host program for a
// sanitizer build:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/overlap_refusals.hip -o overlap_refusals
// It includes geometry.hip itself and stands in for the pools of mpcombi_hip.hip, which a refusal never reaches: every call below must
// come back MPC_ERR_INVALID with a message before a device is selected, so the program needs no GPU and launches nothing.
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
static void expect(const char *what, int rc) {
    const bool ok = rc == MPC_ERR_INVALID && !g_msg.empty();
    std::printf("%-44s rc = %d  %s\n", what, rc, g_msg.c_str());
    if (!ok) ++n_bad;
    g_msg.clear();
}

int main() {
    // heap copies of exactly the sizes the arguments promise: a read past them is the sanitizer's to report
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
    { std::vector<double> bad = ef; bad[4] = std::nan(""); expect("pairs: a non-finite row", pairs(nt, off, bad, a, b, cut, 1e-8)); }
    expect("pairs: a cut row that is not unit", pairs(nt, off, ef, a, b, std::vector<double>{0.0, 2.0, 0.0}, 1e-8));
    expect("split: tol < 0", split(poff, pef, a, b, -1.0));
    expect("split: piece index out of range", split(poff, pef, std::vector<int32_t>{1}, b, 1e-8));
    expect("split: cutter index out of range", split(poff, pef, a, std::vector<int32_t>{2}, 1e-8));
    expect("split: a piece without rows", split(std::vector<int64_t>{0, 0, 4}, pef, std::vector<int32_t>{1}, b, 1e-8));
    { std::vector<double> bad = pef; bad[0] = INFINITY; expect("split: a non-finite piece row", split(poff, bad, a, b, 1e-8)); }
    std::printf("%d unexpected\n", n_bad);
    return n_bad ? 1 : 0;
}
