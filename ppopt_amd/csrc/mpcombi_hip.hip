// mpcombi_hip.hip -- the level engine behind the C ABI (include/mpcombi.h): mpc_handle and everything that needs it, over the
// gfx950 kernels in kernels.hpp / kernels2.hpp; the stages of a large level's host path are level_classic.hpp, those of a level without host round trips (and its batch member) level_small.hpp, those of handle creation create.hpp, the environment knobs knobs.hpp.  The stateless geometry entry points (hit-and-run, slices, point location, search
// trees, closed loop, vertices, merging) are geometry.hip; the LPs, QPs and MIQPs solved at fixed points are points.hip.
//
// Build:  one object per translation unit (this file, geometry.hip, points.hip, batch_level.hip, setup_mfma.hip), linked into
//         libmpcombi_hip.so:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -c <unit>.hip   (__graft_entry__.build)
//
// Host side of the hot path: owns the device-resident program blocks, the frontier (to_check), the pruned list
// (murder_list) and the per-level result buffers; launches the kernels on one HIP stream and times them with HIP
// events.  No CPU fallback exists: without a usable HIP device every entry point fails with MPC_ERR_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <unordered_map>
#include <map>
#include <mutex>
#include <condition_variable>
#include <thread>
#include <functional>
#include <chrono>
#include <atomic>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/mpcombi.h"
#include "kernels.hpp"
#include "kernels2.hpp"
#include "graph.hpp"
#include <memory>

#include "batch_level.hpp"
#include "level_launch.hpp"
#include "setup_mfma.hpp"
#include "host_common.hpp"
#include "knobs.hpp"
#include <rocprim/device/device_radix_sort.hpp>

using namespace mpc;

namespace {
thread_local std::string g_error;
}

// The one definition of what host_common.hpp declares: every translation unit of the library shares these pools.
namespace mpc {

// ---- process-wide recycling of device blocks, pinned host blocks, streams and events -----------------------------------
// A caller that solves many small programs one after the other (the mixed-integer enumeration: one mpc_create /
// mpc_destroy per binary fixation) would otherwise pay ~50 hipMalloc/hipFree, 8 hipHostMalloc/hipHostFree and two
// stream creations per program -- 12 ms, several times the kernel time of such a program.  Blocks are kept in size
// classes (powers of two up to 1 MiB, MiB multiples above) and handed to the next handle on the same device; a block
// is only returned to the pool once the work that used it has completed (destroy synchronises its streams first).
static std::mutex g_dev_pool_mutex;
static std::multimap<std::pair<int, size_t>, void *> g_dev_pool_free;   // (device, size) -> block
static size_t g_dev_pool_bytes = 0;
// Free blocks kept: MPC_DEV_POOL_GB (default 48 -- a sixth of the 288 GB of an MI355X; a batch of 64 sub-programs of the
// mixed-integer enumeration holds ~20 GB of level buffers at once, and the next enumeration takes them over as they are).
static const size_t DEV_POOL_MAX_BYTES = (size_t)(std::max(knob_process("MPC_DEV_POOL_GB"), 0.0) * 1073741824.0);
constexpr size_t DEV_POOL_MAX_BLOCK = size_t(8) << 30;

// size classes: powers of two up to 1 MiB, above that four steps per octave (1, 1.25, 1.5, 1.75 x 2^k: at most 25 % slack, and
// buffers that grow with the level -- a different size at every level of every program -- meet blocks of earlier handles)
size_t dev_size_class(size_t bytes) {
    if (bytes <= 256) return 256;
    if (bytes <= (size_t(1) << 20)) { size_t c = 256; while (c < bytes) c <<= 1; return c; }
    size_t p = size_t(1) << 20;
    while ((p << 1) <= bytes) p <<= 1;
    const size_t step = p >> 2;
    return (bytes + step - 1) / step * step;
}
hipError_t dev_pool_take(size_t cls, void **out) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> lk(g_dev_pool_mutex);
        auto it = g_dev_pool_free.find({dev, cls});
        if (it != g_dev_pool_free.end()) { *out = it->second; g_dev_pool_bytes -= cls; g_dev_pool_free.erase(it); return hipSuccess; }
    }
    hipError_t e = hipMalloc(out, cls);
    if (e != hipSuccess) {   // out of memory: give the pool back to the driver and try once more
        std::vector<void *> drop;
        { std::lock_guard<std::mutex> lk(g_dev_pool_mutex); for (auto &kv : g_dev_pool_free) if (kv.first.first == dev) drop.push_back(kv.second);
          for (auto it = g_dev_pool_free.begin(); it != g_dev_pool_free.end();) { if (it->first.first == dev) { g_dev_pool_bytes -= it->first.second; it = g_dev_pool_free.erase(it); } else ++it; } }
        for (void *q : drop) (void)hipFree(q);
        (void)hipGetLastError();
        e = hipMalloc(out, cls);
    }
    return e;
}
void dev_pool_give(void *p, size_t cls) {
    if (!p) return;
    if (cls <= DEV_POOL_MAX_BLOCK && cls == dev_size_class(cls)) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lk(g_dev_pool_mutex);
        if (g_dev_pool_bytes + cls <= DEV_POOL_MAX_BYTES) { g_dev_pool_free.emplace(std::make_pair(dev, cls), p); g_dev_pool_bytes += cls; return; }
    }
    (void)hipFree(p);
}

// pooled page-locked host memory (also behind mpc_host_alloc / mpc_host_free)
// Two classes of blocks that are never mixed: class 0 = staging for DMA copies (default, coarse-grained mapping); class 1 =
// blocks a RUNNING kernel writes and the host polls (streamed region records, chunk flags, the list-length counters):
// those are allocated hipHostMallocCoherent | hipHostMallocMapped, i.e. fine-grained, so that visibility of the kernel's
// system-scope release does not depend on HIP_HOST_COHERENT or on an undocumented L2 write-back.
static std::mutex g_pool_mutex;
static std::multimap<size_t, void *> g_pool_free[2];       // [class] size -> block
static std::unordered_map<void *, std::pair<size_t, int>> g_pool_live;     // block -> (size, class)
static size_t g_pool_free_bytes = 0;
constexpr size_t POOL_MAX_FREE = size_t(16) << 30;

hipError_t host_pool_take(size_t bytes, void **out, size_t *got, bool coherent) {
    const size_t gran = bytes >= (size_t(1) << 20) ? (size_t(1) << 20) : (size_t(64) << 10);
    const size_t need = std::max<size_t>((bytes + gran - 1) / gran * gran, gran);
    const int cls = coherent ? 1 : 0;
    {
        std::lock_guard<std::mutex> lk(g_pool_mutex);
        auto it = g_pool_free[cls].lower_bound(need);
        if (it != g_pool_free[cls].end() && it->first <= need + need / 2) {
            *out = it->second;
            if (got) *got = it->first;
            g_pool_live[it->second] = {it->first, cls};
            g_pool_free_bytes -= it->first;
            g_pool_free[cls].erase(it);
            return hipSuccess;
        }
    }
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, need, coherent ? (hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) : hipHostMallocPortable);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(g_pool_mutex);
    g_pool_live[p] = {need, cls};
    *out = p;
    if (got) *got = need;
    return hipSuccess;
}
bool host_pool_give(void *p) {
    size_t sz = 0;
    {
        std::lock_guard<std::mutex> lk(g_pool_mutex);
        auto it = g_pool_live.find(p);
        if (it == g_pool_live.end()) return false;
        sz = it->second.first;
        const int cls = it->second.second;
        g_pool_live.erase(it);
        if (g_pool_free_bytes + sz <= POOL_MAX_FREE) {
            g_pool_free[cls].emplace(sz, p);
            g_pool_free_bytes += sz;
            return true;
        }
    }
    (void)hipHostFree(p);
    return true;
}

// streams and events
static std::mutex g_sync_pool_mutex;
static std::map<int, std::vector<hipStream_t>> g_stream_pool;
static std::map<std::pair<int, int>, std::vector<hipEvent_t>> g_event_pool;   // (device, timing?) -> events
static std::map<int, int> g_cu_count;

hipError_t pooled_stream(hipStream_t *out) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> lk(g_sync_pool_mutex);
        auto &v = g_stream_pool[dev];
        if (!v.empty()) { *out = v.back(); v.pop_back(); return hipSuccess; }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
void return_stream(hipStream_t s) {   // synchronised by the caller
    if (!s) return;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_sync_pool_mutex);
    auto &v = g_stream_pool[dev];
    if (v.size() < 1024) v.push_back(s); else (void)hipStreamDestroy(s);   // a stream costs ~3 ms to create and ~2 ms to destroy; a batch of 64 programs holds 200
}
hipError_t pooled_event(hipEvent_t *out, bool timing) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> lk(g_sync_pool_mutex);
        auto &v = g_event_pool[{dev, timing ? 1 : 0}];
        if (!v.empty()) { *out = v.back(); v.pop_back(); return hipSuccess; }
    }
    return timing ? hipEventCreate(out) : hipEventCreateWithFlags(out, hipEventDisableTiming);
}
void return_event(hipEvent_t e, bool timing) {
    if (!e) return;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_sync_pool_mutex);
    auto &v = g_event_pool[{dev, timing ? 1 : 0}];
    if (v.size() < 8192) v.push_back(e); else (void)hipEventDestroy(e);
}
// hipGetDeviceCount costs ~80 us per call on this runtime (it is asked at every mpc_create and every LP batch)
int device_count_cached() {
    static const int n = [] { int v = 0; return hipGetDeviceCount(&v) == hipSuccess ? v : 0; }();
    if (n > 0) return n;
    int v = 0;      // none seen yet: ask again (a device may have been made visible since)
    return hipGetDeviceCount(&v) == hipSuccess ? v : 0;
}
int cu_count(int device) {
    {
        std::lock_guard<std::mutex> lk(g_sync_pool_mutex);
        auto it = g_cu_count.find(device);
        if (it != g_cu_count.end()) return it->second;
    }
    hipDeviceProp_t prop;
    int n = 256;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) n = prop.multiProcessorCount;
    std::lock_guard<std::mutex> lk(g_sync_pool_mutex);
    g_cu_count[device] = n;
    return n;
}

}  // namespace mpc

struct mpc_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // side stream: retry kernels of few long-running wavefronts overlap the main pipeline
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_xfork = nullptr, ev_xjoin = nullptr;
    hipStream_t stream3 = nullptr;   // region stage of a level, launched under its (x,theta) stage
    hipStream_t stream4 = nullptr;   // round 6: k_x1's stream (see ev_x1go)
    // Round 6: the streamed one-step dictionaries of a storing level (k_x1) run on stream4 BESIDE the end of their level (children, pruned
    // masks, counters) and the next level's KKT kernel -- nothing of those reads a dictionary; the first kernel of the next level that
    // does waits for ev_x1done (x1_join).  MPC_X1_DEFER=0: in line, as round 5.  Not when a profile asks for per-kernel event times.
    hipEvent_t ev_x1go = nullptr, ev_x1done = nullptr;
    bool x1_pending = false;
    Knobs kn;                        // what the environment said at creation (knobs.hpp: every member with its variable, its default and its measurements)
    // Round 6: the pruned list bucketed by smallest non-equality member (kernels.hpp, k_children_count_b), rebuilt at the start of every level
    // whose children stage is large enough to pay for it (kn.pruned_bucket_min)
    DevBuf pruned_b, pruned_head;
    hipEvent_t ev_rjoin = nullptr, ev_rgo = nullptr;
    bool r3_dirty = false;           // a region kernel launched on stream3 has not been joined by a completed level yet
    // ---- the region stage of a small level beside the NEXT level's kernels (mpc_solve_start's loop only) ----------------------
    // The region records of a level are output only: the next level needs them for nothing but the verdict "optimal, lower-dimensional"
    // (pruned with its supersets), which no bounded full-dimensional program produces.  A small level therefore generates its children
    // before its regions exist (k_children_count, EXPAND_PENDING), k_region2 runs on stream3 from the theta-stage partition on, and the
    // loop closes the level -- counters, verdicts, record fetch, publication -- behind the NEXT level's closing synchronisation.  A verdict
    // that would not have expanded is a miss: the solve restarts from the root with the deferral switched off for good on this handle.
    // Whatever the launch reads or writes and the next level would overwrite lives in the set's own buffers, swapped with the handle's
    // for the duration of the level (two sets by parity of depth: the next level's launch is queued before this one is closed).
    struct RegionDefer {
        DevBuf kkt_code, kkt_L, part_lists, headd, headi, epool, kept_g, done_g;
        DevBuf dcnt;                 // the level's DCNT_WORDS list lengths (k_region2 reads DC_OPT when each workgroup starts), behind them the launch's own LevelCounters
        hipEvent_t ev_go = nullptr, ev_done = nullptr;   // recorded behind the theta-stage partition (main stream) / behind the launch's publish (stream3)
        bool pending = false;        // launched and not closed
        bool joined = false;         // the next level's children stage (it overwrites the frontier the launch reads) waits for ev_done
        int depth = -1, k = 0, fd = 0, fi = 0, keep_lowdim = 0;
        long long n_opt = 0;
        std::vector<DevBuf *> buffers() { return {&kkt_code, &kkt_L, &part_lists, &headd, &headi, &epool, &kept_g, &done_g, &dcnt}; }
    } rdefer[2];
    int defer_mode = 1;              // mpc_set_region_overlap: 0 never, 1 where a level allows it, 2 (tests): ... and the first close on this handle reports a miss
    bool defer_off = false;          // a deferred region missed on this handle: never again (as no_small_fuse for doubtful candidates)
    bool defer_miss_forced = false;   // (what a level did is in its statistics: mpc_level_stats::region_side_stream 2 / 3)
    static constexpr size_t DEFER_DCNT_BYTES = DCNT_BYTES + sizeof(LevelCounters);
    static constexpr int DEFER_PUB_WORDS = (int)(sizeof(LevelCounters) / 4) + 9;   // k_defer_publish: counters, eight verdict counts, the slots
    // where set i's k_defer_publish writes, in the pinned counter block (cnt_host() below: the level's own words end before byte 1024)
    static_assert(64 + sizeof(LevelCounters) + DCNT_BYTES <= 1024 && DEFER_PUB_WORDS * 4 <= 512 && 1024 + 2 * 512 <= 4096, "the pinned block holds both sets' publishes");
    const unsigned int *defer_pub_host(int i) const { return reinterpret_cast<const unsigned int *>(reinterpret_cast<const char *>(tot_host) + 1024 + 512 * i); }
    unsigned int *defer_pub_dev(int i) const { return reinterpret_cast<unsigned int *>(reinterpret_cast<char *>(tot_dev) + 1024 + 512 * i); }
    bool defer_pending() const { return rdefer[0].pending || rdefer[1].pending; }
    bool theta_open = false;         // the parameter set is open in some direction (or the program has equality rows only): the reference's
                                     // optimality LP can be unbounded -> k_recession behind every verdict stage, no overlapped region launch,
                                     // no level without host round trips, no shared launches
    std::vector<std::pair<void *, size_t>> parked_blocks;   // device blocks the level buffers have outgrown (DevBuf::parked), given back by graveyard_flush
    bool region_side_stream = false; // this level's k_region2 launch ran on the side stream, under the (x,theta) stage (mpc_level_stats)
    bool timing = true;              // mpc_set_timing: HIP-event records around the stages and kernels of a level (off: their times in the stats are 0)
    hipEvent_t ev_part = nullptr;
    long long n_smallpath_doubtful = 0;   // small levels repeated because the fused form met a doubtful candidate
    long long n_smallpath = 0, n_smallpath_fallback = 0;   // levels run that way / of which repeated on the classic path
    DevBuf dcnt;                     // device-resident list lengths of such a level
    int wall_khz = 100000;           // rate of wall_clock64() on the device
    bool own_stream = false;
    int n_cu = 256;
    std::string error;
    std::mutex em;                   // fail() is called by the worker thread and by the caller's thread (mpc_level_chunk_wait)
    // problem
    int n_x = 0, n_t = 0, n_c = 0, n_eq = 0, n_tc = 0, is_qp = 0, kkt_mode = 0;
    int mw = MPC_MASK_WORDS;   // 64-bit words of an active-set mask: 2 (n_c <= 128) or 4 (n_c <= 256)
    DevBuf blocks;            // all read-only problem blocks, one allocation
    DevBuf iblocks;           // integer blocks (row / column maps of the pre-crashed dictionary)
    DevProblem Pv{}, Pr{};    // verdict / region kernel views (same blocks, different LDS layouts)
    int lds_v = 0, lds_r = 0; // dynamic LDS bytes per wavefront
    long long last_level_n = 0;   // candidates of the previous level (= the parents of this one)
    long long n_x1 = 0;       // dictionaries of the last level run that k_x1 wrote
    float ms_x1 = 0;
    long long prev_regions = 0;   // regions the level before found (kn.xq_early_regions compares against it)
    long long n_xq_thread = 0; float ms_xq_thread = 0;   // the last level run: candidates that pass decided, its time
    bool skip_small = false;  // mpc_level_run_batch: this level already went through the no-round-trip launches and has to be repeated classically
    size_t o_elim[6] = {0, 0, 0, 0, 0, 0};   // offsets of Wr, UVr, AATr, Me, Ne, gE in `blocks` (mpc_program_block)
    bool elim_ok = false;     // the blocks with the equality rows eliminated are valid
    int fast = 0;             // 1: register-engine kernels (k_theta2 / k_x2) with k_verdict as the retry path
    int fast_t = 0, fast_x = 0; // instantiation selectors
    long long n_needx = 0;
    DevProblem Pf{};          // view for k_verdict2 (small LDS layout: no tableau)
    int lds_f = 0, grid_f = 0;
    DevBuf retry_list, theta_list, vretry_list, status_tmp, part_counts, part_lists, kept_g, done_g, pf_dev, pr2_dev, headd, headi, epool, facet_flags, kkt_code, kkt_L, theta_blocks, xq_groups, xq_list, x1_buf;
    ThetaArgs targs{};
    // (x,theta) dictionary cache: [0]/[1] ping-pong between the level being read (parents) and the level being written
    DevBuf dict_d[2], dict_i[2], dict_stored[2], parent_slot, parent_slot_next;
    int dict_cur = 0;
    bool have_prev_dict = false, have_parent_slot = false, storing = false;
    long long dict_stride_d = 0, dict_stride_i = 0;

    DevProblem Pr2{};         // view for k_region2
    int lds_r2 = 0, grid_r2 = 0, fast_r = -1;   // fast_r: k_region2 instantiation, -1 = none (n_t == 1 or too many rows)
    bool used_region2 = false;
    long long rretry_rows = -1;      // >= 0: the re-solved candidates' records have been written into their slots on the device (k_rretry_merge); rows of epool in use then (bound)
    long long n_rretry = 0, n_erows = 0;
    int fd = 0, fi = 0;
    HostBuf st_list, st_status, st_hd, st_hi, st_pool, st_fxd, st_fxi, st_rlist;   // pinned staging for region fetches
    int grid_v = 0, grid_r = 0;
    long long rec_d = 0, rec_i = 0;
    // frontier / pruned
    int32_t *tot_host = nullptr, *tot_dev = nullptr;   // 16 counters in pinned host memory that the kernels write directly: list lengths need no copy
    // behind them the closing publish of a level leaves its LevelCounters, and behind those its DCNT_WORDS list lengths (dcnt, words named by DcntWord): these, on the host
    int32_t *cnt_host() const {
        static_assert(sizeof(LevelCounters) % 4 == 0 && sizeof(LevelCounters) + 64 + DCNT_BYTES <= 4096, "LevelCounters + list lengths must fit the pinned block");
        return tot_host + 16 + (int)(sizeof(LevelCounters) / 4);
    }
    const int32_t *opt_ptr = nullptr;                  // list of the optimal candidates of the level (a view, not a copy)
    DevBuf frontier, children, status, pruned, flag, pos, opt_list, childmask, count, offset, recd, reci, ctr, scratch, sums;
    long long n = 0;
    long long n_prev = 0;     // candidates of the level before (0: unknown -- frontier set by the caller)
    int k = 0;
    long long n_pruned = 0;
    long long n_pruned_extra = 0;   // masks added from outside (other ranks') behind this level's own new ones, before mpc_frontier_advance
    // level results
    bool level_done = false;
    long long n_opt = 0, n_children = 0, n_pruned_new = 0, n_regions = 0;
    // ---- region records streamed to the host while the region kernel runs (mpc_level_start with MPC_LEVEL_STREAM) ----
    struct StreamOut {
        void *hd = nullptr, *hi = nullptr, *er = nullptr;   // page-locked blocks the region kernel writes (zero-copy)
        long long n_slots = 0, cap_rows = 0;
        int shift = 8, n_chunks = 0;
        bool active = false;    // this level's records are in these blocks, not in headd / headi / epool
        bool taken = false;     // the caller owns the blocks (mpc_level_stream_info handed them over)
    } so;
    HostBuf st_flags;           // chunk flags (host memory the kernel writes)
    int cw_chunks = 0;          // chunks of the most recent streamed level (mpc_level_chunk_wait keeps working while the worker
                                // already runs the base-set check behind that level, which resets `so`)
    DevBuf chunk_count;
    // ---- worker thread behind mpc_level_start / mpc_level_wait ---------------------------------------------------------
    std::thread worker;
    std::mutex wm;
    std::condition_variable wcv;
    int w_req = 0;              // 0 idle, 1 run a level, 2 exit
    bool w_busy = false, w_stream_ready = false;
    // mirrors of the three flags for a short spin before the condition-variable wait: a hand-over through the condition variable
    // alone costs 20-50 us of GPU idle time per level (tools/gpu_idle.sh), a spinning waiter sees the flag within a microsecond
    std::atomic<int> a_req{0}, a_busy{0}, a_ready{0};
    int w_gen = 0, w_flags = 0, w_rc = 0;
    // result of the base-set check the worker ran behind the last level (MPC_LEVEL_THEN_BASE)
    bool base_valid = false;
    uint8_t base_status = 0;
    long long base_regions = 0;
    std::vector<double> base_rec_d;
    std::vector<int32_t> base_rec_i;
    mpc_level_stats w_stats{};
    // ---- the whole level loop on the worker thread (mpc_solve_start / _level / _chunk_wait / _level_wait / _wait) -----------------
    struct SolveLevel {
        int32_t k = 0, mode = 0, chunk = 0, n_chunks = 0;   // mode: 0 nothing to read, 1 streamed in chunks, 2 complete arrays
        int64_t n = 0, n_slots = 0, n_rows = 0;
        void *hd = nullptr, *hi = nullptr, *er = nullptr;   // page-locked blocks; the caller's once mpc_solve_level has handed them over
        bool handed = false;
        const int32_t *flags = nullptr;                     // chunk flags (valid while the level runs)
        const int32_t *ready_flag = nullptr;                // mode 2, copied by k_fetch_slots: raised (behind head_i, in its block) when the arrays are complete
        mpc_level_stats stats{};
        double ms_wall = 0.0;
        std::atomic<int> ready{0}, done{0};
    };
    std::unique_ptr<SolveLevel[]> sv_levels;                // MPC_MAX_NC + 2 entries, allocated by the first mpc_solve_start
    int sv_max_levels = 0, sv_flags = 0, sv_rc = 0;
    int sv_cur = -1;                                        // level the worker is running (-1: not inside a solve loop)
    std::atomic<int> sv_n{0}, sv_finished{1};               // levels begun so far; the loop has ended
    // ---- connected-graph traversal: wave, visited set and pending neighbours resident on the device (graph.hpp) ----------
    struct GraphState {
        bool active = false;
        int variant = 0;                 // 0 combinatorial_graph, 1 graph
        DevBuf wave, visited, pending, tmp_a, tmp_b, sort_tmp, card, idx, card2, idx2, facet, cnt, off, hist;
        long long n_wave = 0, n_visited = 0, n_pending = 0;
        std::vector<int> gk;             // groups of the current wave: cardinality,
        std::vector<long long> goff, gcnt;   // first mask and number of masks
    } g;
    hipEvent_t ev_hi = nullptr;   // completion of the head_i copy of an asynchronous slot fetch
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t kev[14] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // around k_theta2 / the main k_x2 launch / k_region2 / k_kkt_thread / k_xq / k_xq_thread
};

int mpc::fail(mpc_handle *h, int code, const std::string &msg) {
    if (h) { std::lock_guard<std::mutex> lk(h->em); h->error = msg; } else g_error = msg;
    return code;
}
// the layout of the handle's region records at cardinality k (records.hpp); without k: of the level the handle is at
static RecordShape record_shape(const mpc_handle *h, int k) { return RecordShape{h->n_x, h->n_t, h->n_c, h->n_tc, h->n_eq, k}; }
static RecordShape record_shape(const mpc_handle *h) { return record_shape(h, h->k); }

namespace {

struct Layout { int off_T, off_K, off_L, off_E, off_X, n_doubles, off_as, off_inact, off_colvar, off_rowvar, off_rowkind, off_kept, off_pri, off_stored, n_ints, bytes; };

Layout make_layout(int size_T, int size_K, int size_L, int size_E, int size_X, int kmax, int n_c, int ld_max, int rows_max, int rows_t) {
    Layout l{};
    int o = 0;
    auto take = [&](int sz) { int r = o; o += (sz + 1) & ~1; return r; };
    l.off_T = take(size_T); l.off_K = take(size_K); l.off_L = take(size_L); l.off_E = take(size_E); l.off_X = take(size_X);
    l.n_doubles = o;
    int q = 0;
    auto itake = [&](int sz) { int r = q; q += sz; return r; };
    l.off_as = itake(kmax + 1); l.off_inact = itake(n_c + 1); l.off_colvar = itake(ld_max + 2);
    l.off_rowvar = itake(rows_max + 3); l.off_rowkind = itake(rows_max + 3); l.off_kept = itake(rows_t + 1); l.off_pri = itake(rows_max + 3); l.off_stored = itake(rows_t + 1);
    l.n_ints = q;
    l.bytes = (l.n_doubles * 8 + l.n_ints * 4 + 15) & ~15;
    return l;
}

void apply_layout(DevProblem &P, const Layout &l) {
    P.off_T = l.off_T; P.off_K = l.off_K; P.off_L = l.off_L; P.off_E = l.off_E; P.off_X = l.off_X; P.n_doubles = l.n_doubles;
    P.off_as = l.off_as; P.off_inact = l.off_inact; P.off_colvar = l.off_colvar; P.off_rowvar = l.off_rowvar;
    P.off_rowkind = l.off_rowkind; P.off_kept = l.off_kept; P.off_pri = l.off_pri; P.off_stored = l.off_stored; P.n_ints = l.n_ints;
}

// dense host helpers (one-off program setup; fp64)
// LU with partial pivoting of the n x n matrix M (row major, overwritten); perm receives the row order.
bool lu_factor(std::vector<double> &M, int n, std::vector<int> &perm) {
    perm.resize(n);
    for (int i = 0; i < n; ++i) perm[i] = i;
    double scale = 0;
    for (double v : M) scale = std::max(scale, std::fabs(v));
    for (int c = 0; c < n; ++c) {
        int p = c;
        for (int i = c + 1; i < n; ++i) if (std::fabs(M[(size_t)i * n + c]) > std::fabs(M[(size_t)p * n + c])) p = i;
        if (!(std::fabs(M[(size_t)p * n + c]) > 1e-12 * scale)) return false;
        if (p != c) { for (int j = 0; j < n; ++j) std::swap(M[(size_t)p * n + j], M[(size_t)c * n + j]); std::swap(perm[p], perm[c]); }
        for (int i = c + 1; i < n; ++i) {
            const double f = M[(size_t)i * n + c] / M[(size_t)c * n + c];
            M[(size_t)i * n + c] = f;
            if (f != 0.0) for (int j = c + 1; j < n; ++j) M[(size_t)i * n + j] -= f * M[(size_t)c * n + j];
        }
    }
    return true;
}
void lu_solve_host(const std::vector<double> &LU, const std::vector<int> &perm, int n, const double *rhs, double *x) {
    for (int i = 0; i < n; ++i) { double v = rhs[perm[i]]; for (int l = 0; l < i; ++l) v -= LU[(size_t)i * n + l] * x[l]; x[i] = v; }
    for (int i = n - 1; i >= 0; --i) { double v = x[i]; for (int l = i + 1; l < n; ++l) v -= LU[(size_t)i * n + l] * x[l]; x[i] = v / LU[(size_t)i * n + i]; }
}

}  // namespace

// the buffers a level (re)sizes by its number of candidates: what they outgrow is parked (DevBuf::parked) and given back to the pool by
// graveyard_flush, which the level paths call behind their closing synchronisation (all streams of the handle have been joined by then)
static std::vector<DevBuf *> level_buffers(mpc_handle *h) {
    std::vector<DevBuf *> v = {&h->frontier, &h->children, &h->status, &h->pruned, &h->flag, &h->pos, &h->opt_list, &h->childmask, &h->count, &h->offset, &h->recd, &h->reci,
            &h->sums, &h->retry_list, &h->headd, &h->headi, &h->epool, &h->facet_flags, &h->kkt_code, &h->kkt_L, &h->xq_groups, &h->xq_list, &h->x1_buf, &h->theta_list, &h->vretry_list,
            &h->status_tmp, &h->part_counts, &h->part_lists, &h->kept_g, &h->done_g, &h->dict_d[0], &h->dict_d[1], &h->dict_i[0], &h->dict_i[1],
            &h->dict_stored[0], &h->dict_stored[1], &h->parent_slot, &h->parent_slot_next};
    for (auto &d : h->rdefer) for (DevBuf *b : d.buffers()) v.push_back(b);
    return v;
}
// the handle's three side streams and its events without timing, in the order sync_objects (create.hpp) takes them from the pools and
// mpc_destroy returns them
static std::vector<hipStream_t *> side_streams(mpc_handle *h) { return {&h->stream2, &h->stream3, &h->stream4}; }
static std::vector<hipEvent_t *> untimed_events(mpc_handle *h) {
    return {&h->ev_hi, &h->ev_fork, &h->ev_join, &h->ev_xfork, &h->ev_part, &h->ev_xjoin, &h->ev_x1go, &h->ev_x1done, &h->ev_rjoin, &h->ev_rgo,
            &h->rdefer[0].ev_go, &h->rdefer[0].ev_done, &h->rdefer[1].ev_go, &h->rdefer[1].ev_done};
}
static void graveyard_flush(mpc_handle *h) {
    if (h->defer_pending()) return;   // a region launch beside the next level may still read a block its level has outgrown: kept until a flush behind its close
    for (auto &b : h->parked_blocks) dev_pool_give(b.first, b.second);
    h->parked_blocks.clear();
}
static int create_fill(const mpc_problem *p, int32_t device, void *stream, mpc_handle *h);
static void stream_release(mpc_handle *h);
static void solve_release(mpc_handle *h);
static double batch_level_gb(const mpc_handle *h, int32_t gen_children);
static int fetch_many_wait(int device);
// MPC_BATCH_BUDGET_GB (default 160): device memory the members of one shared launch may hold, read at every call that charges against it
static double batch_budget_gb() { return knob_process("MPC_BATCH_BUDGET_GB"); }
// MPC_DEBUG_MANY=1: the times and misses of mpc_solve_many on stderr; read once, by whichever of its two users comes first
static bool debug_many() { static const bool on = knob_process("MPC_DEBUG_MANY") != 0.0; return on; }
static_assert(XQG_WAVES == 4, "Knobs::xqg_per_cu (knobs.hpp) defaults to XQG_WAVES");

extern "C" {

int mpc_device_count(void) { return device_count_cached(); }

// the build stamp says which binary a record was made with: the compiler's date / time of THIS translation unit (the engine; the
// other units carry no stamp of their own -- __graft_entry__.build prints every object's time) and the hipcc version
#define MPC_STR2(x) #x
#define MPC_STR(x) MPC_STR2(x)
const char *mpc_version(void) {
    return "mpcombi-hip 0.4 (gfx950; built " __DATE__ " " __TIME__ ", hip " MPC_STR(HIP_VERSION_MAJOR) "." MPC_STR(HIP_VERSION_MINOR) "." MPC_STR(HIP_VERSION_PATCH) ")";
}
const char *mpc_last_global_error(void) { return g_error.c_str(); }
const char *mpc_last_error(const mpc_handle *h) { return h ? h->error.c_str() : g_error.c_str(); }

int mpc_create(const mpc_problem *p, int32_t device, void *stream, mpc_handle **out) {
    if (!p || !out) return fail(nullptr, MPC_ERR_INVALID, "null argument");
    *out = nullptr;
    const int nx = p->n_x, nt = p->n_t, nc = p->n_c, ne = p->n_eq, ntc = p->n_tc;
    if (nx < 1 || nt < 1 || nc < 1 || ne < 0 || ne > nc || ntc < 0) return fail(nullptr, MPC_ERR_INVALID, "bad dimensions");
    if (nc > MPC_MAX_NC) return fail(nullptr, MPC_ERR_INVALID, "n_c > 256 is not supported (active sets are bit masks of at most four words)");
    if (nc + ntc + 2 > MPC_MAX_ROWS * 4) return fail(nullptr, MPC_ERR_INVALID, "too many rows");
    if (nt > 64 || nx > 256) return fail(nullptr, MPC_ERR_INVALID, "n_t > 64 or n_x > 256 is not supported");
    if (!p->A || !p->b || !p->F || !p->c || !p->H || (ntc > 0 && (!p->A_t || !p->b_t))) return fail(nullptr, MPC_ERR_INVALID, "null matrix");
    int ndev = 0;
    if ((ndev = device_count_cached()) < 1) return fail(nullptr, MPC_ERR_HIP, "no HIP device available (libmpcombi_hip has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, MPC_ERR_INVALID, "device index out of range");
    // every failure from here on goes through one cleanup path: mpc_destroy returns the handle's streams, events, device
    // blocks and pinned block to the pools (a caller that creates one handle per binary fixation must not leak on OOM)
    mpc_handle *h = new mpc_handle();
    for (DevBuf *b : level_buffers(h)) b->parked = &h->parked_blocks;
    h->dcnt.parked = &h->parked_blocks;   // (swapped with a RegionDefer set's for the duration of a deferring level)
    const int rc_fill = create_fill(p, device, stream, h);
    if (rc_fill != MPC_OK) { (void)mpc_destroy(h); return rc_fill; }
    *out = h;
    return MPC_OK;
}

}  // extern "C"

#include "create.hpp"

// fills a fresh handle: the stages of create.hpp over one CreateRun, in creation's order; on failure the caller destroys it
// (error text in the thread-local g_error, see mpc_last_global_error)
static int create_fill(const mpc_problem *p, int32_t device, void *stream, mpc_handle *h) {
    CreateRun c(p, device, stream, h);
    int rc = c.sync_objects();                      // device, streams and events from the pools, the environment (Knobs)
    if (rc != MPC_OK) return rc;
    c.base_rows();                                  // [b | A | -F ; b_t | 0 | A_t]
    if ((rc = c.base_dictionary()) != MPC_OK) return rc;   // a vertex of the base polytope (one LP), the dictionary there by a fresh LU
    if ((rc = c.theta_vertex()) != MPC_OK) return rc;      // a vertex of the parameter set (one LP, none when n_tc == n_t)
    if ((rc = c.pack_blocks()) != MPC_OK) return rc;       // every read-only block in one allocation, one upload
    if ((rc = c.schur_setup()) != MPC_OK) return rc;       // the MFMA set-up kernel: Schur blocks, kkt_mode, the eliminated blocks
    if ((rc = c.problem_views()) != MPC_OK) return rc;     // DevProblem over the blocks, the integer maps
    if ((rc = c.lds_layouts()) != MPC_OK) return rc;       // Pv, Pr, the 160 KiB check
    if ((rc = c.register_path()) != MPC_OK) return rc;     // the register-resident kernels' selectors; theta_blocks and targs, Pf, then Pr2 (region2_view)
    if ((rc = c.theta_open()) != MPC_OK) return rc;        // open parameter set?  (the bounding box, unless register_path has it)
    return c.records_and_counters();                       // record sizes, counters, the pinned counter block
}

extern "C" {

int mpc_destroy(mpc_handle *h) {
    if (!h) return MPC_OK;
    if (h->worker.joinable()) {
        { std::unique_lock<std::mutex> lk(h->wm); h->wcv.wait(lk, [&] { return !h->w_busy; }); h->w_req = 2; h->a_req.store(1, std::memory_order_release); }
        h->wcv.notify_all();
        h->worker.join();
    }
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->stream2) (void)hipStreamSynchronize(h->stream2);
    if (h->stream3) (void)hipStreamSynchronize(h->stream3);
    if (h->stream4) (void)hipStreamSynchronize(h->stream4);
    graveyard_flush(h);
    for (DevBuf *b : {&h->blocks, &h->iblocks, &h->frontier, &h->children, &h->status, &h->pruned, &h->flag, &h->pos, &h->opt_list,
                      &h->childmask, &h->count, &h->offset, &h->recd, &h->reci, &h->ctr, &h->pruned_b, &h->pruned_head, &h->scratch, &h->sums, &h->retry_list, &h->pf_dev, &h->pr2_dev, &h->headd, &h->headi, &h->epool, &h->facet_flags, &h->kkt_code, &h->kkt_L, &h->theta_blocks, &h->xq_groups, &h->xq_list, &h->x1_buf, &h->theta_list, &h->vretry_list, &h->status_tmp, &h->part_counts, &h->part_lists, &h->kept_g, &h->done_g, &h->dict_d[0], &h->dict_d[1], &h->dict_i[0], &h->dict_i[1],
                      &h->dict_stored[0], &h->dict_stored[1], &h->parent_slot, &h->parent_slot_next, &h->dcnt}) b->release();
    for (auto &d : h->rdefer) for (DevBuf *b : d.buffers()) b->release();
    if (h->tot_host) { (void)host_pool_give(h->tot_host); h->tot_host = h->tot_dev = nullptr; }
    for (HostBuf *b : {&h->st_list, &h->st_status, &h->st_hd, &h->st_hi, &h->st_pool, &h->st_fxd, &h->st_fxi, &h->st_rlist, &h->st_flags}) b->release();
    stream_release(h);
    solve_release(h);
    h->chunk_count.release();
    for (DevBuf *b : {&h->g.wave, &h->g.visited, &h->g.pending, &h->g.tmp_a, &h->g.tmp_b, &h->g.sort_tmp, &h->g.card, &h->g.idx, &h->g.card2, &h->g.idx2, &h->g.facet, &h->g.cnt, &h->g.off, &h->g.hist}) b->release();
    for (auto &e : h->ev) return_event(e, true);
    for (auto &e : h->kev) return_event(e, true);
    for (hipEvent_t *e : untimed_events(h)) return_event(*e, false);
    for (hipStream_t *s : side_streams(h)) return_stream(*s);
    if (h->own_stream) return_stream(h->stream);
    delete h;
    return MPC_OK;
}

// Gives the level buffers of an idle handle (frontier, children, statuses, lists, region records, both generations of the dictionary
// cache, the pruned list ...) back to the pool: the program's own blocks stay, a later level allocates again.  For a driver that holds
// many handles at once (mpc_level_run_batch) and wants the memory of those that are finished for the ones that are not.
int mpc_trim(mpc_handle *h) {
    if (!h) return MPC_ERR_INVALID;
    { std::lock_guard<std::mutex> lk(h->wm); if (h->w_busy) return fail(h, MPC_ERR_STATE, "a level started with mpc_level_start is still running"); }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->stream2) HIP_TRY(h, hipStreamSynchronize(h->stream2));
    if (h->stream3) HIP_TRY(h, hipStreamSynchronize(h->stream3));
    if (h->stream4) HIP_TRY(h, hipStreamSynchronize(h->stream4));
    h->x1_pending = false;
    graveyard_flush(h);
    stream_release(h);
    for (DevBuf *b : {&h->frontier, &h->children, &h->status, &h->pruned, &h->flag, &h->pos, &h->opt_list, &h->childmask, &h->count, &h->offset, &h->recd, &h->reci,
                      &h->sums, &h->retry_list, &h->headd, &h->headi, &h->epool, &h->facet_flags, &h->kkt_code, &h->kkt_L, &h->xq_groups, &h->xq_list, &h->x1_buf, &h->theta_list, &h->vretry_list,
                      &h->status_tmp, &h->part_counts, &h->part_lists, &h->kept_g, &h->done_g, &h->dict_d[0], &h->dict_d[1], &h->dict_i[0], &h->dict_i[1],
                      &h->dict_stored[0], &h->dict_stored[1], &h->parent_slot, &h->parent_slot_next}) b->release();
    for (auto &d : h->rdefer) for (DevBuf *b : d.buffers()) b->release();
    for (HostBuf *b : {&h->st_list, &h->st_status, &h->st_hd, &h->st_hi, &h->st_pool, &h->st_fxd, &h->st_fxi, &h->st_rlist, &h->st_flags}) b->release();
    h->n = 0; h->k = 0; h->n_pruned = 0; h->n_pruned_extra = 0; h->level_done = false;
    h->have_prev_dict = false; h->have_parent_slot = false;
    return MPC_OK;
}
// Device memory (GB) the next level of the handle's frontier will hold on the no-round-trip path (buffers sized by the number of
// candidates: region records, children, two generations of the dictionary cache): what mpc_level_batch_start charges against
// MPC_BATCH_BUDGET_GB.
double mpc_level_memory_gb(const mpc_handle *h, int32_t gen_children) { return h ? batch_level_gb(h, gen_children) : 0.0; }

int32_t mpc_mask_words(const mpc_handle *h) { return h ? h->mw : MPC_MASK_WORDS; }
int mpc_program_block(mpc_handle *h, int32_t which, double *out, int64_t cap, int64_t *n_out) {
    if (!h || !n_out) return MPC_ERR_INVALID;
    const long long nc = h->n_c, nx = h->n_x, nr = h->n_t + 1;
    const double *src = nullptr;
    long long n = 0;
    switch (which) {
        case 0: src = h->Pv.W; n = nc * nc; break;
        case 1: src = h->Pv.UV; n = nc * nr; break;
        case 2: src = h->Pv.Gt; n = nc * nx; break;
        case 3: src = h->Pv.X0H; n = nx * nr; break;
        case 4: src = h->Pv.AAT; n = nc * nc; break;
        // blocks with the equality rows eliminated (setup_mfma.hpp); empty when the program has none or the elimination is off
        case 5: src = h->blocks.as<double>() + h->o_elim[0]; n = nc * nc; break;
        case 6: src = h->blocks.as<double>() + h->o_elim[1]; n = nc * nr; break;
        case 7: src = h->blocks.as<double>() + h->o_elim[2]; n = nc * nc; break;
        case 8: src = h->blocks.as<double>() + h->o_elim[3]; n = (long long)h->n_eq * nr; break;
        case 9: src = h->blocks.as<double>() + h->o_elim[4]; n = (long long)h->n_eq * nc; break;
        case 10: src = h->blocks.as<double>() + h->o_elim[5]; n = 2LL * h->n_eq; break;
        default: return fail(h, MPC_ERR_INVALID, "mpc_program_block: which must be 0..10");
    }
    if (which < 4 && h->kkt_mode != 0) n = 0;   // the Schur blocks exist only for a positive definite Q
    if (which >= 5 && !h->elim_ok) n = 0;
    *n_out = n;
    if (n == 0) return MPC_OK;
    if (!out || cap < n) return fail(h, MPC_ERR_CAPACITY, "mpc_program_block: buffer too small");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(out, src, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPC_OK;
}
int mpc_set_region_overlap(mpc_handle *h, int32_t on) {
    if (!h || on < 0 || on > 3) return MPC_ERR_INVALID;
    h->kn.no_roverlap = on == 0;
    h->defer_mode = (on == 0 || on == 2) ? 0 : (on == 3 ? 2 : 1);   // (a miss already met stays: defer_off)
    return MPC_OK;
}
int mpc_set_timing(mpc_handle *h, int32_t on) { if (!h) return MPC_ERR_INVALID; h->timing = on; return MPC_OK; }
int64_t mpc_region_doubles(const mpc_handle *h) { return h ? h->rec_d : 0; }
int64_t mpc_region_ints(const mpc_handle *h) { return h ? h->rec_i : 0; }
int32_t mpc_lds_bytes(const mpc_handle *h, int32_t which) { return !h ? 0 : (which == 0 ? h->lds_v : h->lds_r); }
void *mpc_stream(const mpc_handle *h) { return h ? reinterpret_cast<void *>(h->stream) : nullptr; }

// ---- frontier ----------------------------------------------------------------------------------------------
static int frontier_reset(mpc_handle *h, long long n, int k) {
    if (n < 0 || k < 0 || (n > 0 && k > h->n_c)) return fail(h, MPC_ERR_INVALID, "bad frontier shape");
    if (n > 0x7fffffffLL / std::max(k + 1, 1)) return fail(h, MPC_ERR_INVALID, "frontier too large for 32-bit offsets");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->frontier.ensure((size_t)std::max<long long>(n, 1) * std::max(k, 1) * sizeof(int32_t), h->stream));
    h->n = n; h->k = k; h->level_done = false; h->n_pruned_extra = 0; h->n_prev = 0; h->prev_regions = 0;
    h->have_prev_dict = false; h->have_parent_slot = false;   // a frontier set from outside has no cached parent dictionaries
    return MPC_OK;
}

int mpc_frontier_root(mpc_handle *h) {
    if (!h) return MPC_ERR_INVALID;
    const int cnt = h->n_c - h->n_eq;
    int rc = frontier_reset(h, cnt, h->n_eq + 1);
    if (rc) return rc;
    if (cnt > 0) hipLaunchKernelGGL(k_root_frontier, dim3((cnt + 63) / 64), dim3(64), 0, h->stream, h->n_eq, h->n_c, h->frontier.as<int32_t>());
    HIP_TRY(h, hipGetLastError());
    return MPC_OK;
}

int mpc_frontier_set(mpc_handle *h, const int32_t *cand, int64_t n, int32_t k) {
    if (!h || (!cand && n > 0 && k > 0)) return MPC_ERR_INVALID;
    int rc = frontier_reset(h, n, k);
    if (rc) return rc;
    if (n > 0 && k > 0) {
        HIP_TRY(h, hipMemcpyAsync(h->frontier.p, cand, (size_t)n * k * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return MPC_OK;
}

int mpc_frontier_set_device(mpc_handle *h, const int32_t *cand, int64_t n, int32_t k) {
    if (!h || (!cand && n > 0 && k > 0)) return MPC_ERR_INVALID;
    int rc = frontier_reset(h, n, k);
    if (rc) return rc;
    if (n > 0 && k > 0) {
        HIP_TRY(h, hipMemcpyAsync(h->frontier.p, cand, (size_t)n * k * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));  // caller-owned source
    }
    return MPC_OK;
}

int mpc_frontier_shard(mpc_handle *h, int32_t rank, int32_t world) {
    if (!h || world < 1 || rank < 0 || rank >= world) return MPC_ERR_INVALID;
    if (world == 1) return MPC_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const long long n = h->n, n_new = n > rank ? (n - rank + world - 1) / world : 0;
    const int k = h->k;
    hipStream_t st = h->stream;
    if (n_new > 0 && k > 0) {
        HIP_TRY(h, h->children.ensure((size_t)n_new * k * sizeof(int32_t), st));
        const long long tot = n_new * k;
        hipLaunchKernelGGL(k_take_rows, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, h->frontier.as<int32_t>(), n_new, k, (long long)rank,
                           (long long)world, h->children.as<int32_t>());
        HIP_TRY(h, hipGetLastError());
        std::swap(h->frontier, h->children);
        if (h->have_parent_slot) {
            HIP_TRY(h, h->parent_slot_next.ensure((size_t)n_new * sizeof(int32_t), st));
            hipLaunchKernelGGL(k_take_rows, dim3((unsigned)((n_new + 255) / 256)), dim3(256), 0, st, h->parent_slot.as<int32_t>(), n_new, 1, (long long)rank,
                               (long long)world, h->parent_slot_next.as<int32_t>());
            HIP_TRY(h, hipGetLastError());
            std::swap(h->parent_slot, h->parent_slot_next);
        }
        HIP_TRY(h, hipStreamSynchronize(st));
    }
    h->n = n_new;
    h->n_prev = 0;   // h->children no longer holds the previous level's frontier (k_xq_thread's look-up of other parents is off for this level)
    h->level_done = false;
    return MPC_OK;
}

int mpc_frontier_info(const mpc_handle *h, int64_t *n, int32_t *k) {
    if (!h) return MPC_ERR_INVALID;
    if (n) *n = h->n;
    if (k) *k = h->k;
    return MPC_OK;
}

int mpc_frontier_get(mpc_handle *h, int32_t *cand, int64_t cap) {
    if (!h || !cand) return MPC_ERR_INVALID;
    if (cap < h->n) return fail(h, MPC_ERR_CAPACITY, "frontier buffer too small");
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->n > 0 && h->k > 0) {
        HIP_TRY(h, hipMemcpyAsync(cand, h->frontier.p, (size_t)h->n * h->k * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return MPC_OK;
}

int mpc_pruned_clear(mpc_handle *h) { if (!h) return MPC_ERR_INVALID; h->n_pruned = 0; h->n_pruned_extra = 0; return MPC_OK; }

static int pruned_add(mpc_handle *h, const uint64_t *masks, int64_t m, hipMemcpyKind kind) {
    if (!h || (m > 0 && !masks) || m < 0) return MPC_ERR_INVALID;
    if (m == 0) return MPC_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    // A level that has run keeps its newly pruned masks right behind the list (they join it at mpc_frontier_advance): masks that
    // arrive in between -- the other ranks' -- go behind those.
    const long long tail = h->level_done ? h->n_pruned_new + h->n_pruned_extra : 0;
    HIP_TRY(h, h->pruned.ensure((size_t)(h->n_pruned + tail + m) * h->mw * sizeof(uint64_t), h->stream, true));
    HIP_TRY(h, hipMemcpyAsync(h->pruned.as<uint64_t>() + (size_t)(h->n_pruned + tail) * h->mw, masks, (size_t)m * h->mw * sizeof(uint64_t), kind, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // caller-owned source
    if (h->level_done) h->n_pruned_extra += m; else h->n_pruned += m;
    return MPC_OK;
}
int mpc_pruned_add(mpc_handle *h, const uint64_t *masks, int64_t m) { return pruned_add(h, masks, m, hipMemcpyHostToDevice); }
int mpc_pruned_add_device(mpc_handle *h, const uint64_t *masks, int64_t m) { return pruned_add(h, masks, m, hipMemcpyDeviceToDevice); }
int64_t mpc_pruned_count(const mpc_handle *h) { return h ? h->n_pruned : 0; }
int mpc_pruned_get(mpc_handle *h, uint64_t *masks, int64_t cap) {
    if (!h || !masks) return MPC_ERR_INVALID;
    if (cap < h->n_pruned) return fail(h, MPC_ERR_CAPACITY, "pruned buffer too small");
    if (h->n_pruned > 0) {
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipMemcpyAsync(masks, h->pruned.p, (size_t)h->n_pruned * h->mw * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return MPC_OK;
}

// exclusive scan of n int32 values on the handle's stream (three launches); *total_dev receives the sum
static int launch_scan(mpc_handle *h, const int32_t *in, int32_t *out, long long n, int32_t *total_dev) {
    if (n <= SMALL_LEVEL_N) {   // one single-block launch
        hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(SCAN_BLOCK), 0, h->stream, in, out, (int)n, total_dev);
        HIP_TRY(h, hipGetLastError());
        return MPC_OK;
    }
    const int nb = (int)((n + SCAN_BLOCK - 1) / SCAN_BLOCK);
    HIP_TRY(h, h->sums.ensure((size_t)std::max(nb, 1) * sizeof(int32_t), h->stream));
    // four-wavefront workgroups (see block_exclusive_scan_it)
    hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(SCAN_BLOCK / SCAN_IT), 0, h->stream, in, n, h->sums.as<int32_t>());
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SCAN_BLOCK / SCAN_IT), 0, h->stream, h->sums.as<int32_t>(), nb, total_dev);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(SCAN_BLOCK / SCAN_IT), 0, h->stream, in, out, n, h->sums.as<int32_t>());
    HIP_TRY(h, hipGetLastError());
    return MPC_OK;
}

// LDS-engine region kernel over `list` (n_list optimal candidates), fixed-stride records at slots 0..n_list-1.
// Few candidates: one wavefront per (candidate, facet) and an assembly pass (latency form); many: one per candidate.
static int launch_region_v1(mpc_handle *h, const int32_t *list, long long n_list, int k, LevelCounters *ctr) {
    hipStream_t st = h->stream;
    HIP_TRY(h, h->recd.ensure((size_t)n_list * h->rec_d * sizeof(double), st));
    HIP_TRY(h, h->reci.ensure((size_t)n_list * h->rec_i * sizeof(int32_t), st));
    const long long rows_t = h->n_c - h->n_eq + h->n_tc;
    const bool split = h->n_t > 1 && rows_t > 0 && n_list <= 2LL * h->grid_r;
    HIP_TRY(h, hipMemsetAsync(&ctr->work_region, 0, sizeof(unsigned int), st));
    if (split) {
        HIP_TRY(h, h->facet_flags.ensure((size_t)n_list * rows_t, st));
        hipLaunchKernelGGL((k_region<RG_FACET>), dim3((unsigned)std::max<long long>(1, std::min<long long>(n_list * rows_t, 4LL * h->grid_r))), dim3(64), h->lds_r, st, h->Pr,   // (a program without inactive rows: rows_t = 0)
                           h->frontier.as<int32_t>(), k, list, (int)n_list, h->status.as<uint8_t>(), h->recd.as<double>(), h->reci.as<int32_t>(),
                           h->rec_d, h->rec_i, ctr, h->facet_flags.as<uint8_t>());
        HIP_TRY(h, hipMemsetAsync(&ctr->work_region, 0, sizeof(unsigned int), st));
        hipLaunchKernelGGL((k_region<RG_ASSEMBLE>), dim3((unsigned)std::min<long long>(n_list, h->grid_r)), dim3(64), h->lds_r, st, h->Pr,
                           h->frontier.as<int32_t>(), k, list, (int)n_list, h->status.as<uint8_t>(), h->recd.as<double>(), h->reci.as<int32_t>(),
                           h->rec_d, h->rec_i, ctr, h->facet_flags.as<uint8_t>());
    } else {
        hipLaunchKernelGGL((k_region<RG_FULL>), dim3((unsigned)std::min<long long>(n_list, h->grid_r)), dim3(64), h->lds_r, st, h->Pr,
                           h->frontier.as<int32_t>(), k, list, (int)n_list, h->status.as<uint8_t>(), h->recd.as<double>(), h->reci.as<int32_t>(),
                           h->rec_d, h->rec_i, ctr, (uint8_t *)nullptr);
    }
    HIP_TRY(h, hipGetLastError());
    return MPC_OK;
}

// ---- one level ------------------------------------------------------------------------------------------------
// tells a caller blocked in mpc_level_stream_info that the region stage of the running level has been launched (or that
// this level does not stream)
static void stream_ready(mpc_handle *h) {
    if (h->sv_cur >= 0) {
        // inside mpc_solve_start's loop: the region stage of level sv_cur has been launched -- its page-locked arrays are handed to
        // the caller of mpc_solve_level right away (a level that does not stream is published by the loop itself, after its fetch)
        auto &lv = h->sv_levels[h->sv_cur];
        if (h->so.active && !h->so.taken && !lv.ready.load(std::memory_order_relaxed)) {
            lv.mode = 1; lv.hd = h->so.hd; lv.hi = h->so.hi; lv.er = h->so.er;
            lv.n_slots = h->so.n_slots; lv.n_rows = h->so.cap_rows; lv.chunk = 1 << h->so.shift; lv.n_chunks = h->so.n_chunks;
            lv.flags = h->st_flags.as<int32_t>();
            h->so.taken = true;
            lv.ready.store(1, std::memory_order_release);
            { std::lock_guard<std::mutex> lk(h->wm); }
            h->wcv.notify_all();
        }
        return;
    }
    std::lock_guard<std::mutex> lk(h->wm);
    h->w_stream_ready = true;
    h->a_ready.store(1, std::memory_order_release);
    h->wcv.notify_all();
}
static void stream_release(mpc_handle *h) {   // blocks of a streamed level nobody took
    // a level that ended early (error return) after launching its region kernel on stream3 may still be writing the blocks
    if (h->r3_dirty) { (void)hipStreamSynchronize(h->stream3); if (h->stream4) (void)hipStreamSynchronize(h->stream4); h->r3_dirty = false; }
    if (!h->so.taken) { if (h->so.hd) (void)host_pool_give(h->so.hd); if (h->so.hi) (void)host_pool_give(h->so.hi); if (h->so.er) (void)host_pool_give(h->so.er); }
    h->so = mpc_handle::StreamOut();
}

// ---- what the three forms of a level (no round trips: level_small.hpp, its batch member, classic: level_classic.hpp) share besides their
// kernels (level_launch.hpp) and the names of their list lengths (DcntWord, batch_level.hpp) ------------------------------------------------
// Largest number of inequality rows k_kkt_thread solves for (one thread per candidate, everything in registers).  Round 6: 8 -> 10 -- the
// K = 9, 10 instantiations keep their k x k system and the k x (n_theta + 1) multipliers in 234-256 VGPRs (+ up to 108 AGPRs as spill space,
// one wavefront per SIMD at n_theta > 4) and still beat the wavefront-wide LDS solve inside k_theta2 several times over; K = 12
// needs 364 registers at every n_theta.  The shared launches of several programs (batch_level.hip) keep 8.
constexpr int KKT_THREAD_MAX = 10;
constexpr int KKT_SPREAD = BATCH_KKT_SPREAD, KKT_SPREAD_KMAX = BATCH_KKT_SPREAD_KMAX;   // small levels: lanes per candidate of k_kkt_thread, up to this many inequality rows
// every stream of the handle that may read or write dictionary records waits for the deferred k_x1 of the previous level (stream waits: the host does not block)
static int x1_join(mpc_handle *h) {
    if (!h->x1_pending) return MPC_OK;
    for (hipStream_t sx : {h->stream, h->stream2, h->stream3}) if (sx) HIP_TRY(h, hipStreamWaitEvent(sx, h->ev_x1done, 0));
    h->x1_pending = false;
    return MPC_OK;
}
// shape of the level's region records (doubles / ints per slot) and the region stage's per-level state
static void level_record_shape(mpc_handle *h, int k) {
    h->used_region2 = false; h->n_rretry = 0; h->n_erows = 0; h->rretry_rows = -1;
    const RecordShape sh = record_shape(h, k);
    h->fd = sh.fd(); h->fi = sh.fi();
}
// partition spec of k_partition_small / k_part_*: status -> class nibble, 15 = none
static unsigned long long part_spec(std::initializer_list<std::pair<int, int>> classes) {
    unsigned long long spec = ~0ull;
    for (const auto &sc : classes) spec = (spec & ~(15ull << (4 * sc.first))) | ((unsigned long long)sc.second << (4 * sc.first));
    return spec;
}
static int dict_nxc(const mpc_handle *h) { return h->fast_x >= 2 ? 32 : 16; }   // dictionary columns k_x2 keeps
// does a level of nn candidates keep its dictionaries for its children?  (one record per candidate, within dict_budget_gb)
static bool dict_will_store(const mpc_handle *h, size_t nn, int32_t gen_children) {
    const int nxc = dict_nxc(h);
    const double need_gb = (double)nn * ((long long)nxc * h->Pf.n_d0r * 8.0 + dict_ints(h->Pf.n_d0r, nxc, h->n_c) * 4.0) / 1e9;
    return gen_children && need_gb <= h->kn.dict_budget_gb;
}
// The dictionary cache of a level's (x,theta) stage: record strides, the previous level's records if its children know their parent
// slots, and -- if the level stores (h->storing) -- this level's buffers.  The clearing of dict_stored[dict_cur] is the caller's.
static int dict_cache_begin(mpc_handle *h, size_t nn, int32_t gen_children, hipStream_t st, DictCache &dc) {
    const int nxc = dict_nxc(h);
    h->dict_stride_d = (long long)nxc * h->Pf.n_d0r;   // column-major tableau
    h->dict_stride_i = dict_ints(h->Pf.n_d0r, nxc, h->n_c);
    dc = DictCache{};
    dc.fresh_limit = h->kn.x_fresh_limit; dc.second_max = h->kn.x_second_max;
    dc.stride_d = h->dict_stride_d; dc.stride_i = h->dict_stride_i;
    if (h->have_prev_dict && h->have_parent_slot) {
        dc.parent_slot = h->parent_slot.as<int32_t>();
        dc.prev_d = h->dict_d[1 - h->dict_cur].as<double>(); dc.prev_i = h->dict_i[1 - h->dict_cur].as<int32_t>();
    }
    h->storing = false;
    if (dict_will_store(h, nn, gen_children)) {
        HIP_TRY(h, h->dict_d[h->dict_cur].ensure(nn * h->dict_stride_d * sizeof(double), st));
        HIP_TRY(h, h->dict_i[h->dict_cur].ensure(nn * h->dict_stride_i * sizeof(int32_t), st));
        HIP_TRY(h, h->dict_stored[h->dict_cur].ensure(nn, st));
        dc.cur_d = h->dict_d[h->dict_cur].as<double>(); dc.cur_i = h->dict_i[h->dict_cur].as<int32_t>(); dc.stored = h->dict_stored[h->dict_cur].as<uint8_t>();
        h->storing = true;
    }
    return MPC_OK;
}
// the end of a level that ran to its end (behind its closing synchronisation; not on a path's fallback return)
static void level_close(mpc_handle *h, long long n) { graveyard_flush(h); h->level_done = true; h->last_level_n = n; stream_ready(h); }
// bytes of one dictionary record that are actually moved: the used columns (value + D0 columns) and the integer part
// (what k_x2 reads of a record; the stored record also carries the children's look-up bytes)
static long long dict_record_bytes(const mpc_handle *h) { return (long long)(h->Pf.n_d0c + 1) * h->Pf.n_d0r * 8 + (long long)dict_ints_head(h->Pf.n_d0r, dict_nxc(h)) * 4; }
// the statistics every form of a level reports alike; the caller adds its own (times, work-item counts, dictionary traffic)
static void level_stats_common(const mpc_handle *h, const LevelCounters &host_ctr, mpc_level_stats *stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->n = h->n; stats->k = h->k; stats->kkt_mode = h->kkt_mode;
    for (int i = 0; i < 6; ++i) stats->n_status[i] = (int64_t)host_ctr.status[i];
    stats->n_regions = h->n_regions; stats->n_children = h->n_children; stats->n_pruned_new = h->n_pruned_new;
    stats->lp_pivots = (int64_t)host_ctr.pivots; stats->n_xtheta_fallback = (int64_t)host_ctr.xtheta_fallbacks;
    for (int i = 0; i < 4; ++i) stats->wave_cycles[i] = (int64_t)host_ctr.cycles[i];
    stats->n_x_cached = (int64_t)host_ctr.x_cached; stats->n_region_rows = h->n_erows; stats->n_opt = h->n_opt; stats->xq_pivots = (int64_t)host_ctr.xq_pivots;
    stats->xq_record_ints = dict_ints_head(h->Pf.n_d0r, dict_nxc(h)) - 1; stats->xq_record_rows = h->Pf.n_d0r; stats->xq_record_cols = h->Pf.n_d0c + 1;
}

// the level without host round trips and its batch form: level_run_small, batch_prepare / batch_finish, defer_swap / defer_join / defer_drain
#include "level_small.hpp"

static int level_run_impl(mpc_handle *h, int32_t gen_children, int32_t flags, mpc_level_stats *stats);

// device memory one member's level holds on the no-round-trip path (the buffers are sized by the bound n): region records, children,
// two generations of the dictionary cache
static double batch_level_gb(const mpc_handle *h, int32_t gen_children) {
    const double n = (double)h->n;
    const int k = h->k;
    const RecordShape sh = record_shape(h, k);
    double bytes = n * ((double)sh.fd() * 8.0 + (double)sh.fi() * 4.0 + (double)sh.rows_t() * sh.row_len() * 8.0);
    if (gen_children) bytes += n * std::max(h->n_c - k, 1) * (k + 2) * 4.0;
    const double nxc = h->fast_x >= 2 ? 32 : 16;
    bytes += 2.0 * n * (nxc * h->Pf.n_d0r * 8.0 + (2.0 * h->Pf.n_d0r + nxc + 4) * 4.0);
    return bytes / 1e9;
}

struct BatchToken {
    std::vector<mpc_handle *> hs;
    std::vector<int32_t> gen;
    int32_t flags = 0;
    std::vector<BatchMember> members;
    std::vector<int> alone;      // members outside the shared launches: run one after the other by mpc_level_run's own paths
    hipStream_t st = nullptr;
    DevBuf tab_dev;              // the members' argument table the launches read (one per batch call: concurrent batches do not share it)
    HostBuf tab_host;
    ~BatchToken() { tab_dev.release(); tab_host.release(); }   // only after the launches have completed (wait) or were never queued
};

int mpc_level_batch_start(mpc_handle **hs, int32_t n_handles, const int32_t *gen_children, int32_t flags, void **token) {
    if (!hs || n_handles <= 0 || !gen_children || !token) return MPC_ERR_INVALID;
    *token = nullptr;
    mpc_handle *h0 = hs[0];
    if (!h0) return MPC_ERR_INVALID;
    for (int i = 0; i < n_handles; ++i) {
        mpc_handle *h = hs[i];
        if (!h) return MPC_ERR_INVALID;
        if (h->device != h0->device) return fail(h, MPC_ERR_INVALID, "mpc_level_run_batch: the members must live on one device");
        if (flags & MPC_LEVEL_GRAPH) return fail(h, MPC_ERR_INVALID, "mpc_level_run_batch: MPC_LEVEL_GRAPH is not a batch level");
        { std::lock_guard<std::mutex> lk(h->wm); if (h->w_busy) return fail(h, MPC_ERR_STATE, "a level started with mpc_level_start is still running"); }
        { std::lock_guard<std::mutex> lk(h->wm); h->w_stream_ready = false; h->a_ready.store(0, std::memory_order_release); }
    }
    {
        std::vector<mpc_handle *> sorted(hs, hs + n_handles);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(h0, MPC_ERR_INVALID, "mpc_level_run_batch: a handle appears twice");
    }
    HIP_TRY(h0, hipSetDevice(h0->device));
    if (fetch_many_wait(h0->device) != MPC_OK) return fail(h0, MPC_ERR_HIP, "mpc_level_batch_start: the shared record copy (k_fetch_many) failed");   // the members' record buffers are free again
    std::unique_ptr<BatchToken> t(new BatchToken());
    t->hs.assign(hs, hs + n_handles);
    t->gen.assign(gen_children, gen_children + n_handles);
    t->flags = flags & ~(MPC_LEVEL_THEN_BASE | MPC_LEVEL_ONLY_BASE | MPC_LEVEL_STREAM);
    t->members.reserve(n_handles);
    const double budget_gb = batch_budget_gb();
    double used_gb = 0.0;
    for (int i = 0; i < n_handles; ++i) {
        mpc_handle *h = hs[i];
        stream_release(h);
        { int rcj = x1_join(h); if (rcj) return rcj; }
        // MPC_SMALLPATH_MAX bounds the single-program path only (above it the overlapped classic path is faster for ONE program)
        const long long keep_max = h->kn.smallpath_max;
        // (bounded: the shared launches compact / partition / scan a member with single 1024-thread blocks -- beyond 2^18 candidates a
        // member takes its turn alone, on the multi-block kernels of the classic path)
        h->kn.smallpath_max = std::max<long long>(keep_max, 1LL << 18);
        const bool ok = small_path_ok(h, h->n, h->k, t->flags, gen_children[i]);
        h->kn.smallpath_max = keep_max;
        bool ok_i = ok;
        if (ok_i) {
            // MPC_BATCH_BUDGET_GB (default 160 of the 288 GB): members beyond it take their turn after the shared launches, one at a time
            const double gb = batch_level_gb(h, gen_children[i]);
            if (used_gb + gb > budget_gb && !t->members.empty()) ok_i = false; else used_gb += gb;
        }
        if (!ok_i) { t->alone.push_back(i); HIP_TRY(h, hipStreamSynchronize(h->stream)); continue; }   // (copies of the last level's records: complete when this call returns, as for the members)
        BatchMember m;
        const int rc = batch_prepare(h, gen_children[i], t->flags, m);
        if (rc != MPC_OK) return rc;
        m.id = i;
        t->members.push_back(m);
    }
    if (!t->members.empty()) {
        mpc_handle *hl = hs[t->members[0].id];     // ids are the caller's positions (batch_level_launch reorders the members)
        t->st = hl->stream;
        const int lead = t->members[0].id;
        if (hl->timing) HIP_TRY(hl, hipEventRecord(hl->ev[0], t->st));
        const size_t tab_bytes = t->members.size() * sizeof(BatchMember);
        HIP_TRY(hl, t->tab_dev.ensure(tab_bytes, t->st));
        HIP_TRY(hl, t->tab_host.ensure(tab_bytes));
        hipError_t e = batch_level_launch(t->members.data(), (int)t->members.size(), t->st, t->tab_host.as<BatchMember>(), t->tab_dev.as<BatchMember>());
        if (e != hipSuccess) { (void)hipStreamSynchronize(t->st); return fail(hl, MPC_ERR_HIP, std::string("batch level launch: ") + hipGetErrorString(e)); }   // (what was queued still reads the table)
        if (hl->timing) HIP_TRY(hl, hipEventRecord(hl->ev[3], t->st));
        t->alone.insert(t->alone.begin(), -1 - lead);      // first entry < 0: the member whose events bracket the launches
    }
    *token = t.release();
    return MPC_OK;
}

int mpc_level_batch_wait(void *token, mpc_level_stats *stats, int32_t *n_batched) {
    if (!token) return MPC_ERR_INVALID;
    std::unique_ptr<BatchToken> t(static_cast<BatchToken *>(token));
    if (n_batched) *n_batched = 0;
    if (!t->members.empty()) {
        const int lead = -1 - t->alone.front();
        t->alone.erase(t->alone.begin());
        mpc_handle *hl = t->hs[lead];
        HIP_TRY(hl, hipSetDevice(hl->device));
        HIP_TRY(hl, hipStreamSynchronize(t->st));   // the level's only synchronisation, for all members
        float ms = 0;
        if (hl->timing) HIP_TRY(hl, hipEventElapsedTime(&ms, hl->ev[0], hl->ev[3]));
        for (const BatchMember &m : t->members) {
            bool fallback = false;
            const int rc = batch_finish(t->hs[m.id], t->gen[m.id], m, ms, stats ? stats + m.id : nullptr, &fallback);
            if (rc != MPC_OK) return rc;
            if (fallback) {
                // The member ran in the shared launches: m_children_write has overwritten the previous level's frontier in h->children,
                // which the classic path's search for other parents (k_xq_thread, alt.prev_frontier) would walk with the wrong row width.
                // As in level_run_small's repeat: no other-parent look-ups on the repeated level.  (Members that never ran keep n_prev.)
                t->hs[m.id]->n_prev = 0;
                t->alone.push_back(m.id);
            }
            else if (n_batched) ++*n_batched;
        }
    }
    for (int i : t->alone) {
        mpc_handle *h = t->hs[i];
        h->skip_small = true;
        const int rc = level_run_impl(h, t->gen[i], t->flags, stats ? stats + i : nullptr);
        h->skip_small = false;
        if (rc != MPC_OK) return rc;
    }
    return MPC_OK;
}

int mpc_level_run_batch(mpc_handle **hs, int32_t n_handles, const int32_t *gen_children, int32_t flags, mpc_level_stats *stats, int32_t *n_batched) {
    void *token = nullptr;
    const int rc = mpc_level_batch_start(hs, n_handles, gen_children, flags, &token);
    if (rc != MPC_OK) return rc;
    return mpc_level_batch_wait(token, stats, n_batched);
}

#include "level_classic.hpp"

static int level_run_impl(mpc_handle *h, int32_t gen_children, int32_t flags, mpc_level_stats *stats) {
    if (!h) return MPC_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    stream_release(h);
    // (a deferred k_x1 of the previous level: joined at once unless this is a large level whose first kernel, k_kkt_thread, reads no dictionary)
    const bool x1_late_join = h->x1_pending && h->fast && !h->kn.force_v1 && h->kkt_mode == 0 && h->kn.no_kkt_thread != 1 &&
                              (h->skip_small || !small_path_ok(h, h->n, h->k, flags, gen_children)) && h->k - h->targs.ne >= 1 && h->k - h->targs.ne <= KKT_THREAD_MAX;
    if (!x1_late_join) { int rcj = x1_join(h); if (rcj) return rcj; }
    if (!h->skip_small && small_path_ok(h, h->n, h->k, flags, gen_children)) {
        bool fallback = false;
        const int rcs = level_run_small(h, gen_children, flags, stats, &fallback);
        if (rcs != MPC_OK || !fallback) return rcs;
    }
    h->region_side_stream = false;
    h->n_opt = h->n_children = h->n_pruned_new = h->n_regions = 0;
    h->n_needx = 0;
    h->n_xq_thread = 0; h->ms_xq_thread = 0;
    // the classic path: the stages of level_classic.hpp over one LevelRun, in the level's order
    LevelRun lv(h, gen_children, flags);
    if (lv.n > 0) {
        if (int rc = lv.begin()) return rc;                            // buffers, counters cleared, pruned buckets
        if (h->fast && !h->kn.force_v1) {
            if (int rc = lv.kkt_stage()) return rc;                    // k_kkt_thread
            if (int rc = lv.early_thread_pass()) return rc;            // last level: k_xq_thread on stream2, beside ...
            if (int rc = lv.theta_stage()) return rc;                  // ... k_theta2
            if (int rc = lv.first_partition()) return rc;              // x_first (the plans queued at once) / early_xq / plain: the level's first read-back
            if (int rc = lv.doubtful_side_stream()) return rc;         // k_verdict on stream2
            if (int rc = lv.overlapped_region_launch()) return rc;     // k_region2 on stream3, under the (x,theta) stage
            if (int rc = lv.open_list()) return rc;                    // join of the early thread pass; what is still open
            if (int rc = lv.quick_test()) return rc;                   // last level: k_xq_thread, k_xq / k_xq_grouped
            if (int rc = lv.x_stage()) return rc;                      // plans + k_x1 + k_x2, or k_x2
            if (int rc = lv.second_partition_and_tail()) return rc;    // behind an overlapped region launch: the speculative end of the level
            if (int rc = lv.retry_and_late()) return rc;               // doubtful candidates re-solved, late optimal candidates
        } else {
            if (int rc = lv.plain_verdict()) return rc;                // k_verdict for every candidate
        }
        if (int rc = lv.region_stage()) return rc;                     // k_region2 in line, k_region for what it gave up on
        if (int rc = lv.tail()) return rc;                             // pruned masks, children, histogram, publish; the closing synchronisation
        if (int rc = lv.read_back()) return rc;                        // counters, event times, debug prints
    }
    level_close(h, lv.n);
    if (stats) lv.fill_stats(stats);
    return MPC_OK;
}

int mpc_level_run(mpc_handle *h, int32_t gen_children, mpc_level_stats *stats) { return mpc_level_run_ex(h, gen_children, 0, stats); }
int mpc_level_run_ex(mpc_handle *h, int32_t gen_children, int32_t flags, mpc_level_stats *stats) {
    if (!h) return MPC_ERR_INVALID;
    if ((flags & MPC_LEVEL_GRAPH) && gen_children) return fail(h, MPC_ERR_INVALID, "MPC_LEVEL_GRAPH has no children");
    { std::lock_guard<std::mutex> lk(h->wm); if (h->w_busy) return fail(h, MPC_ERR_STATE, "a level started with mpc_level_start is still running"); }
    // MPC_LEVEL_STREAM is honoured here too: the region kernel then writes its records into page-locked host memory and
    // mpc_level_stream_info hands the (complete) arrays over after this call -- no device-to-host fetch for small levels
    { std::lock_guard<std::mutex> lk(h->wm); h->w_stream_ready = false; h->a_ready.store(0, std::memory_order_release); }
    return level_run_impl(h, gen_children, flags & ~(MPC_LEVEL_THEN_BASE | MPC_LEVEL_ONLY_BASE), stats);
}

// ---- the same level, driven by the handle's worker thread ---------------------------------------------------------------
// the level's region records off the device: sizes, SlotFetch and the slot / compact / fixed fetches, the shared copy launches
#include "level_fetch.hpp"

// The base active set (the equality rows alone; driver :142-146) on the worker thread.  Any failure simply leaves the check to the caller.
static void worker_base_check(mpc_handle *h) {
    std::vector<int32_t> base((size_t)std::max(h->n_eq, 1));
    for (int i = 0; i < h->n_eq; ++i) base[(size_t)i] = i;
    mpc_level_stats bs;
    std::memset(&bs, 0, sizeof(bs));
    h->base_rec_d.assign((size_t)h->rec_d, 0.0);
    h->base_rec_i.assign((size_t)h->rec_i, -1);
    int64_t cand = 0;
    int rb = mpc_frontier_set(h, base.data(), 1, h->n_eq);
    if (rb == MPC_OK) { h->n_pruned = 0; rb = level_run_impl(h, 0, 0, &bs); }
    if (rb == MPC_OK) rb = mpc_level_status(h, &h->base_status);
    if (rb == MPC_OK && bs.n_regions > 0) rb = mpc_level_regions(h, h->base_rec_d.data(), h->base_rec_i.data(), &cand, 1);
    if (rb == MPC_OK) { h->base_regions = bs.n_regions; h->base_valid = true; }
}

// a level of the solve loop back to "not run": blocks nobody took go back to the pool, nothing is known of the level any more
static void solve_level_reset(mpc_handle::SolveLevel &lv) {
    if (!lv.handed) { if (lv.hd) (void)host_pool_give(lv.hd); if (lv.hi) (void)host_pool_give(lv.hi); if (lv.er) (void)host_pool_give(lv.er); }
    lv.hd = lv.hi = lv.er = nullptr; lv.handed = false; lv.flags = nullptr; lv.ready_flag = nullptr; lv.mode = 0;
    lv.ready.store(0, std::memory_order_release); lv.done.store(0, std::memory_order_release);
}
// blocks of levels of the previous solve loop that nobody took
static void solve_release(mpc_handle *h) {
    if (!h->sv_levels) return;
    const int nl = h->sv_n.load(std::memory_order_acquire);
    // a level's k_fetch_slots is queued behind that level's closing synchronisation: a block nobody took may still be written to
    // (abandoned solve restarted at once) -- the stream is drained before such a block goes back to the pool
    bool pending = false;
    for (int i = 0; i < nl; ++i) {
        const auto &lv = h->sv_levels[i];
        if (!lv.handed && lv.ready_flag && !__atomic_load_n(lv.ready_flag, __ATOMIC_ACQUIRE)) pending = true;
    }
    if (pending && h->stream) (void)hipStreamSynchronize(h->stream);
    for (int i = 0; i < nl; ++i) solve_level_reset(h->sv_levels[i]);
    h->sv_n.store(0, std::memory_order_release);
}

// The records of the level that has just run in line (not deferred), where the region kernel has not streamed them into lv's blocks already.
static int solve_fetch_level(mpc_handle *h, mpc_handle::SolveLevel &lv, int flags) {
    if (lv.ready.load(std::memory_order_relaxed)) {
        if (lv.stats.n_region_retry == 0) return MPC_OK;
        // candidates the LDS-engine kernel re-solved after the stream: their slots are filled in place (the caller lists the level
        // again after mpc_solve_level_wait)
        int64_t ns = 0, nr = 0;
        return level_regions_slots_impl(h, static_cast<double *>(lv.hd), static_cast<int32_t *>(lv.hi), lv.n_slots, static_cast<double *>(lv.er), lv.n_rows, &ns, &nr, FetchMode::in_place);
    }
    // the level did not stream (no optimal candidate; run without host round trips, its records in device buffers; LDS-engine
    // region kernel; > 1 GiB of records): fetched here, complete when published
    if (!((flags & MPC_SOLVE_FETCH) && lv.stats.n_regions > 0 && h->n_opt > 0 && !h->so.active)) { lv.mode = 0; return MPC_OK; }
    int64_t ns = 0, nr = 0;
    const RecordSizes z = level_record_sizes(h);
    const size_t b_er = (size_t)std::max<long long>(z.rows_cap, 1) * (h->n_t + 1) * sizeof(double);
    if (h->used_region2 && h->n_rretry == 0)   // every record is in slot form on the device
        // (the counter: DC_FETCH_COUNTER, a list length the level's own kernels are taken not to use, cleared with the others at its start)
        return solve_fetch_slots(h, lv, z.n_slots, z.fd, z.fi, h->n_erows, b_er, h->headd.p, h->headi.p, h->epool.p, reinterpret_cast<unsigned int *>(h->dcnt.as<int32_t>() + DC_FETCH_COUNTER));
    int rc = MPC_OK;
    const size_t b_hd = (size_t)z.n_slots * z.fd * sizeof(double), b_hi = (size_t)z.n_slots * z.fi * sizeof(int32_t);
    if (host_pool_take(b_hd, &lv.hd, nullptr, false) != hipSuccess || host_pool_take(b_hi + 64, &lv.hi, nullptr, false) != hipSuccess ||
        host_pool_take(b_er, &lv.er, nullptr, false) != hipSuccess) rc = fail(h, MPC_ERR_HIP, "mpc_solve: page-locked memory for a level's region records");
    if (rc == MPC_OK)
        rc = level_regions_slots_impl(h, static_cast<double *>(lv.hd), static_cast<int32_t *>(lv.hi), z.n_slots, static_cast<double *>(lv.er), z.rows_cap, &ns, &nr, FetchMode::complete);
    lv.mode = 2; lv.n_slots = ns; lv.n_rows = nr; lv.chunk = 0; lv.n_chunks = 0;
    return rc;
}
static void solve_publish(mpc_handle *h, mpc_handle::SolveLevel &lv) {
    lv.ready.store(1, std::memory_order_release);
    lv.done.store(1, std::memory_order_release);
    { std::lock_guard<std::mutex> lk(h->wm); }
    h->wcv.notify_all();
}

// Closes a level whose region launch ran beside the level after it (mpc_handle::RegionDefer): behind that level's closing synchronisation
// (its children stage waited for the launch), or at once (`final`) when the loop ends with the launch pending.  *miss: a slot's verdict
// would not have expanded as its candidate did -- nothing is published, the caller abandons the pass.  Otherwise the level's statistics
// get what the launch counted, the records are fetched and the level is published as a level in line is.
static int defer_close(mpc_handle *h, mpc_handle::RegionDefer &d, int flags, bool final, bool *miss) {
    *miss = false;
    const int set = (int)(&d - h->rdefer);
    auto &lv = h->sv_levels[d.depth];
    HIP_TRY(h, hipEventSynchronize(d.ev_done));
    d.pending = false;
    const unsigned int *pub = h->defer_pub_host(set);
    LevelCounters rc;
    std::memcpy(&rc, pub, sizeof(LevelCounters));
    const unsigned int *verdict = pub + sizeof(LevelCounters) / 4;   // [0..7] slots by head_i[slot][0], [8] slots
    long long n_slots = 0;
    for (int i = 0; i < 8; ++i) n_slots += verdict[i];
    if ((long long)verdict[8] != d.n_opt || n_slots != d.n_opt) return fail(h, MPC_ERR_STATE, "defer_close: the deferred region launch did not write one record per optimal candidate");
    const bool forced = h->defer_mode == 2 && !h->defer_miss_forced;
    if (forced) h->defer_miss_forced = true;
    // what k_small_end would have pruned, what k_region2 gave up on (the LDS-engine region kernel is no part of the small path), and an
    // mpLP candidate that is expanded as a feasible one after all (its children pass the filter an optimal parent's do not)
    if (forced || rc.n_rretry > 0 || verdict[ST_RETRY] > 0 || verdict[ST_INFEASIBLE] > 0 || (verdict[ST_OPT_NO_REGION] > 0 && !d.keep_lowdim) ||
        (verdict[ST_FEASIBLE] > 0 && !h->is_qp)) {
        *miss = true;
        return MPC_OK;
    }
    mpc_level_stats &st = lv.stats;
    for (int i = 0; i < 6; ++i) st.n_status[i] += (int64_t)verdict[i];
    st.n_regions = (int64_t)verdict[ST_REGION];
    st.n_region_rows = (int64_t)rc.e_rows;
    st.lp_pivots += (int64_t)rc.pivots;
    st.wave_cycles[3] += (int64_t)rc.cycles[3];
    if (d.n_opt > 0 && rc.r2_t1 > ~rc.r2_not_t0 && h->wall_khz > 0) st.ms_region2 = (float)((double)(rc.r2_t1 - ~rc.r2_not_t0) / (double)h->wall_khz);
    int rcs = MPC_OK;
    if ((flags & MPC_SOLVE_FETCH) && st.n_regions > 0) {
        // (st: the level's own k and n_opt, the launch's regions and rows; no candidate re-solved.  Regions without a single row: the block
        // is sized as for a level that pools nothing, n_regions * rows_t rows, where one row would do)
        const RecordSizes z = level_record_sizes(h, st);
        rcs = solve_fetch_slots(h, lv, z.n_slots, z.fd, z.fi, (long long)rc.e_rows, (size_t)std::max<long long>(z.rows_cap, 1) * (h->n_t + 1) * sizeof(double),
                                d.headd.p, d.headi.p, d.epool.p, reinterpret_cast<unsigned int *>(d.dcnt.as<int32_t>() + DC_FETCH_COUNTER));
    } else lv.mode = 0;
    if (rcs == MPC_OK && final) {
        // no level followed: the handle is left as a level in line leaves it (mpc_level_status, mpc_level_regions_* after mpc_solve_wait)
        defer_swap(h, d);
        h->n_regions = st.n_regions; h->n_erows = (long long)rc.e_rows;
        if (d.n_opt > 0) {
            hipLaunchKernelGGL(k_defer_status, dim3((unsigned)((d.n_opt + 255) / 256)), dim3(256), 0, h->stream, h->headi.as<int32_t>(), d.fi, (int)d.n_opt, h->status.as<uint8_t>());
            HIP_TRY(h, hipGetLastError());
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (rcs != MPC_OK) return rcs;
    solve_publish(h, lv);
    return MPC_OK;
}
// A deferred region launch of level `from` missed: every launch is waited for, the handle never defers again, and what the abandoned pass
// has made known of the levels from `from` on (a streamed level after it may have handed its blocks to sv_levels already; the consumer
// takes levels in order and is still waiting for `from`) is taken back.
static void defer_abandon(mpc_handle *h, int from) {
    (void)hipStreamSynchronize(h->stream);
    defer_drain(h);
    h->defer_off = true;
    const int nl = h->sv_n.load(std::memory_order_acquire);
    for (int i = from; i < nl; ++i) solve_level_reset(h->sv_levels[i]);
}

// The level loop of the reference's driver (mp_solvers/mpqp_parrallel_combinatorial.py:98-139) on the worker thread: root frontier,
// then level after level -- run, publish the level's records, advance the frontier -- without a hand-over to the caller in between.
// A small level may leave its region launch running beside the level after it (RegionDefer): that level is published one level later,
// by defer_close.  After a miss the loop starts again from the root: the levels below the one that missed are final and published (the
// path is deterministic) -- they are run again for the handle's state alone (`replay_below`).
static int worker_solve(mpc_handle *h) {
    const int flags = h->sv_flags;
    const int level_flags = flags & (MPC_LEVEL_STREAM | MPC_LEVEL_KEEP_LOWDIM);
    int rc = MPC_OK, replay_below = 0, missed = -1;
    for (;;) {
        int miss_at = -1;
        rc = mpc_pruned_clear(h);
        if (rc == MPC_OK) rc = mpc_frontier_root(h);
        for (int depth = 0; rc == MPC_OK && depth < h->sv_max_levels; ++depth) {
            const int gen = depth + 1 != h->sv_max_levels;
            if (depth < replay_below) {
                mpc_level_stats rs{};
                h->sv_cur = depth;
                rc = level_run_impl(h, gen, level_flags & ~MPC_LEVEL_STREAM, &rs);
                h->sv_cur = -1;
                if (rc != MPC_OK || !gen || rs.n_children == 0) break;
                rc = mpc_frontier_advance(h);
                continue;
            }
            auto &lv = h->sv_levels[depth];
            lv.k = h->k; lv.n = h->n;
            const auto t0 = std::chrono::steady_clock::now();
            h->sv_cur = depth;
            if (h->sv_n.load(std::memory_order_relaxed) < depth + 1) h->sv_n.store(depth + 1, std::memory_order_release);
            rc = level_run_impl(h, gen, level_flags, &lv.stats);
            auto &mine = h->rdefer[depth & 1], &before = h->rdefer[(depth + 1) & 1];
            const bool deferred = rc == MPC_OK && mine.pending && mine.depth == depth;
            if (rc == MPC_OK && depth == missed) lv.stats.region_side_stream = 3;   // its deferred launch missed: this is the repeat, in line
            if (rc == MPC_OK && before.pending) {
                // this level's closing synchronisation has passed, its children stage waited for the launch of the level before
                bool miss = false;
                rc = defer_close(h, before, flags, false, &miss);
                if (rc == MPC_OK && miss) { miss_at = before.depth; break; }
            }
            if (rc == MPC_OK && !deferred) rc = solve_fetch_level(h, lv, flags);
            lv.ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            h->sv_cur = -1;
            if (rc != MPC_OK) break;
            if (!deferred) solve_publish(h, lv);
            if (!gen || lv.stats.n_children == 0) {
                if (deferred) {   // the loop ends with the launch pending: closed at once
                    bool miss = false;
                    rc = defer_close(h, mine, flags, true, &miss);
                    if (rc == MPC_OK && miss) miss_at = depth;
                }
                break;
            }
            rc = mpc_frontier_advance(h);
        }
        h->sv_cur = -1;
        if (miss_at < 0 || rc != MPC_OK) break;
        defer_abandon(h, miss_at);
        replay_below = missed = miss_at;
    }
    defer_drain(h);   // (an error inside the loop)
    h->base_valid = false;
    if (rc == MPC_OK && (flags & MPC_LEVEL_THEN_BASE)) worker_base_check(h);
    return rc;
}

static void worker_main(mpc_handle *h) {
    for (;;) {
        int gen = 0, flags = 0, req = 0;
        {
            for (int spin = 0; spin < 20000 && !h->a_req.load(std::memory_order_acquire); ++spin) __builtin_ia32_pause();
            std::unique_lock<std::mutex> lk(h->wm);
            h->wcv.wait(lk, [&] { return h->w_req != 0; });
            if (h->w_req == 2) return;
            req = h->w_req; gen = h->w_gen; flags = h->w_flags; h->w_req = 0; h->a_req.store(0, std::memory_order_release);
        }
        mpc_level_stats st;
        std::memset(&st, 0, sizeof(st));
        if (req == 3) {
            const int rcs = worker_solve(h);
            {
                std::lock_guard<std::mutex> lk(h->wm);
                h->sv_rc = rcs; h->w_rc = rcs; h->w_stats = st; h->w_busy = false; h->w_stream_ready = true;
                h->sv_finished.store(1, std::memory_order_release);
                h->a_ready.store(1, std::memory_order_release); h->a_busy.store(0, std::memory_order_release);
            }
            h->wcv.notify_all();
            continue;
        }
        const bool only_base = (flags & MPC_LEVEL_ONLY_BASE) != 0;
        const int rc = only_base ? MPC_OK : level_run_impl(h, gen, flags, &st);
        h->base_valid = false;
        // only when the level's records were streamed AND the caller already owns the arrays (or the level has no region at all): a
        // level that did not stream (LDS-engine region kernel ...) is fetched by the caller after mpc_level_wait, from the very state
        // this check would replace
        const bool streamed_and_taken = h->so.active && h->so.taken;
        if (rc == MPC_OK && (only_base || ((flags & MPC_LEVEL_THEN_BASE) && !gen && st.n_region_retry == 0 && (streamed_and_taken || st.n_regions == 0))))
            worker_base_check(h);   // right behind the last level, while the caller is still turning the streamed records into objects
        {
            std::lock_guard<std::mutex> lk(h->wm);
            h->w_rc = rc; h->w_stats = st; h->w_busy = false; h->w_stream_ready = true;
            h->a_ready.store(1, std::memory_order_release); h->a_busy.store(0, std::memory_order_release);
        }
        h->wcv.notify_all();
    }
}

int mpc_level_start(mpc_handle *h, int32_t gen_children, int32_t flags) {
    if (!h) return MPC_ERR_INVALID;
    std::unique_lock<std::mutex> lk(h->wm);
    if (h->w_busy) return fail(h, MPC_ERR_STATE, "mpc_level_start: the previous level has not been waited for");
    if (!h->worker.joinable()) h->worker = std::thread(worker_main, h);
    h->w_gen = gen_children; h->w_flags = flags; h->w_busy = true; h->w_stream_ready = false; h->w_req = 1;
    h->a_busy.store(1, std::memory_order_release); h->a_ready.store(0, std::memory_order_release); h->a_req.store(1, std::memory_order_release);
    lk.unlock();
    h->wcv.notify_all();
    return MPC_OK;
}

int mpc_level_stream_info(mpc_handle *h, double **head_d, int32_t **head_i, double **erows, int64_t *n_slots, int64_t *cap_rows,
                          int32_t *chunk, int32_t *n_chunks) {
    if (!h) return MPC_ERR_INVALID;
    std::unique_lock<std::mutex> lk(h->wm);
    if (!h->w_busy && !h->w_stream_ready) return fail(h, MPC_ERR_STATE, "mpc_level_stream_info without a level started by mpc_level_start");
    if (!h->w_stream_ready) {
        lk.unlock();
        for (int spin = 0; spin < 200000 && !h->a_ready.load(std::memory_order_acquire); ++spin) __builtin_ia32_pause();
        lk.lock();
    }
    h->wcv.wait(lk, [&] { return h->w_stream_ready; });
    auto &so = h->so;
    const bool on = so.active && !so.taken;
    if (head_d) *head_d = on ? static_cast<double *>(so.hd) : nullptr;
    if (head_i) *head_i = on ? static_cast<int32_t *>(so.hi) : nullptr;
    if (erows) *erows = on ? static_cast<double *>(so.er) : nullptr;
    if (n_slots) *n_slots = on ? so.n_slots : 0;
    if (cap_rows) *cap_rows = on ? so.cap_rows : 0;
    if (chunk) *chunk = on ? (1 << so.shift) : 0;
    if (n_chunks) *n_chunks = on ? so.n_chunks : 0;
    if (on) so.taken = true;   // the three blocks now belong to the caller (mpc_host_free)
    return MPC_OK;
}

int mpc_level_chunk_wait(mpc_handle *h, int32_t j) {
    if (!h || j < 0 || j >= h->cw_chunks || !h->st_flags.p) return MPC_ERR_INVALID;
    const int32_t *flag = h->st_flags.as<int32_t>() + j;
    for (unsigned spin = 0;; ++spin) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE)) return MPC_OK;
        if ((spin & 1023u) == 1023u) {
            // the level has ended (normally or with an error) without raising the flag: do not wait for ever
            bool busy;
            { std::lock_guard<std::mutex> lk(h->wm); busy = h->w_busy; }
            if (!busy) return __atomic_load_n(flag, __ATOMIC_ACQUIRE) ? MPC_OK : fail(h, MPC_ERR_STATE, "mpc_level_chunk_wait: the level ended without completing this chunk");
        }
        __builtin_ia32_pause();
    }
}

int mpc_level_wait(mpc_handle *h, mpc_level_stats *stats) {
    if (!h) return MPC_ERR_INVALID;
    std::unique_lock<std::mutex> lk(h->wm);
    if (!h->worker.joinable()) return fail(h, MPC_ERR_STATE, "mpc_level_wait without mpc_level_start");
    if (h->w_busy) {
        lk.unlock();
        for (int spin = 0; spin < 200000 && h->a_busy.load(std::memory_order_acquire); ++spin) __builtin_ia32_pause();
        lk.lock();
    }
    h->wcv.wait(lk, [&] { return !h->w_busy; });
    if (stats) *stats = h->w_stats;
    return h->w_rc;
}

// ---- the whole level loop behind one call ---------------------------------------------------------------------------------------
int mpc_solve_start(mpc_handle *h, int32_t max_levels, int32_t flags) {
    if (!h || max_levels < 0) return MPC_ERR_INVALID;
    std::unique_lock<std::mutex> lk(h->wm);
    if (h->w_busy) return fail(h, MPC_ERR_STATE, "mpc_solve_start: the previous level / solve has not been waited for");
    if (!h->sv_levels) h->sv_levels.reset(new mpc_handle::SolveLevel[MPC_MAX_NC + 2]);
    solve_release(h);
    h->sv_max_levels = std::min<int>(max_levels, MPC_MAX_NC + 1); h->sv_flags = flags; h->sv_rc = MPC_OK;
    h->sv_finished.store(0, std::memory_order_release);
    if (!h->worker.joinable()) h->worker = std::thread(worker_main, h);
    h->w_gen = 0; h->w_flags = flags; h->w_busy = true; h->w_stream_ready = false; h->w_req = 3;
    h->a_busy.store(1, std::memory_order_release); h->a_ready.store(0, std::memory_order_release); h->a_req.store(1, std::memory_order_release);
    lk.unlock();
    h->wcv.notify_all();
    return MPC_OK;
}

// waits (short spin, then the condition variable) until pred() holds
static void solve_wait_for(mpc_handle *h, const std::function<bool()> &pred) {
    for (int spin = 0; spin < 400000; ++spin) { if (pred()) return; __builtin_ia32_pause(); }
    std::unique_lock<std::mutex> lk(h->wm);
    h->wcv.wait(lk, pred);
}

int mpc_solve_level(mpc_handle *h, int32_t level, mpc_solve_level_info *info) {
    if (!h || !info || level < 0 || !h->sv_levels || level > MPC_MAX_NC) return MPC_ERR_INVALID;
    auto &lv = h->sv_levels[level];
    solve_wait_for(h, [&] { return lv.ready.load(std::memory_order_acquire) != 0 || h->sv_finished.load(std::memory_order_acquire) != 0; });
    std::memset(info, 0, sizeof(*info));
    info->level = level;
    if (!lv.ready.load(std::memory_order_acquire)) { info->mode = -1; return h->sv_rc; }   // the loop ended before (or inside) this level
    if (lv.mode == 2 && lv.ready_flag) {
        // the arrays are being written by k_fetch_slots on the handle's stream: its last workgroup raises the flag
        for (unsigned spin = 0; !__atomic_load_n(lv.ready_flag, __ATOMIC_ACQUIRE); ++spin) {
            if ((spin & 4095u) == 4095u && h->sv_finished.load(std::memory_order_acquire)) {
                if (h->sv_rc != MPC_OK) { info->mode = -1; return h->sv_rc; }
                // the loop has ended without an error: the copy kernel is queued on the handle's stream -- once that stream has drained the
                // flag is either up or will never be (a launch that failed later than hipGetLastError could see)
                (void)hipSetDevice(h->device);
                const hipError_t es = hipStreamSynchronize(h->stream);
                if (es != hipSuccess || !__atomic_load_n(lv.ready_flag, __ATOMIC_ACQUIRE)) {
                    info->mode = -1;
                    return fail(h, es != hipSuccess ? MPC_ERR_HIP : MPC_ERR_STATE, "mpc_solve_level: the solve ended without completing this level's record copy");
                }
            }
            __builtin_ia32_pause();
        }
    }
    info->k = lv.k; info->n = lv.n; info->mode = lv.mode; info->chunk = lv.chunk; info->n_chunks = lv.n_chunks;
    info->n_slots = lv.n_slots; info->n_rows = lv.n_rows;
    if (lv.mode != 0 && !lv.handed) {
        info->head_d = static_cast<double *>(lv.hd); info->head_i = static_cast<int32_t *>(lv.hi); info->erows = static_cast<double *>(lv.er);
        lv.handed = true;   // the three blocks now belong to the caller (mpc_host_free)
    } else if (lv.mode != 0) return fail(h, MPC_ERR_STATE, "mpc_solve_level: the arrays of this level have been handed over already");
    return MPC_OK;
}

int mpc_solve_chunk_wait(mpc_handle *h, int32_t level, int32_t j) {
    if (!h || level < 0 || !h->sv_levels || level > MPC_MAX_NC) return MPC_ERR_INVALID;
    auto &lv = h->sv_levels[level];
    if (lv.mode != 1 || j < 0 || j >= lv.n_chunks) return MPC_ERR_INVALID;
    for (unsigned spin = 0;; ++spin) {
        // a finished level has every chunk complete (and its flag words may already belong to the next level)
        if (lv.done.load(std::memory_order_acquire)) return MPC_OK;
        if (__atomic_load_n(lv.flags + j, __ATOMIC_ACQUIRE)) return MPC_OK;
        if ((spin & 1023u) == 1023u && h->sv_finished.load(std::memory_order_acquire))
            return lv.done.load(std::memory_order_acquire) ? MPC_OK : fail(h, MPC_ERR_STATE, "mpc_solve_chunk_wait: the solve ended without completing this chunk");
        __builtin_ia32_pause();
    }
}

int mpc_solve_level_wait(mpc_handle *h, int32_t level, mpc_level_stats *stats, double *ms_wall) {
    if (!h || level < 0 || !h->sv_levels || level > MPC_MAX_NC) return MPC_ERR_INVALID;
    auto &lv = h->sv_levels[level];
    solve_wait_for(h, [&] { return lv.done.load(std::memory_order_acquire) != 0 || h->sv_finished.load(std::memory_order_acquire) != 0; });
    if (!lv.done.load(std::memory_order_acquire)) return h->sv_rc != MPC_OK ? h->sv_rc : fail(h, MPC_ERR_STATE, "mpc_solve_level_wait: the solve ended before this level");
    if (stats) *stats = lv.stats;
    if (ms_wall) *ms_wall = lv.ms_wall;
    return MPC_OK;
}

int mpc_solve_wait(mpc_handle *h, int32_t *n_levels) {
    if (!h) return MPC_ERR_INVALID;
    if (!h->worker.joinable() || !h->sv_levels) return fail(h, MPC_ERR_STATE, "mpc_solve_wait without mpc_solve_start");
    {
        std::unique_lock<std::mutex> lk(h->wm);
        if (h->w_busy) {
            lk.unlock();
            for (int spin = 0; spin < 200000 && h->a_busy.load(std::memory_order_acquire); ++spin) __builtin_ia32_pause();
            lk.lock();
        }
        h->wcv.wait(lk, [&] { return !h->w_busy; });
    }
    if (n_levels) {
        int nl = 0;
        while (nl < h->sv_n.load(std::memory_order_acquire) && h->sv_levels[nl].done.load(std::memory_order_acquire)) ++nl;
        *n_levels = nl;
    }
    return h->sv_rc;
}

int mpc_base_result(mpc_handle *h, uint8_t *status, int64_t *n_regions, double *rec_d, int32_t *rec_i) {
    if (!h) return MPC_ERR_INVALID;
    { std::lock_guard<std::mutex> lk(h->wm); if (h->w_busy) return fail(h, MPC_ERR_STATE, "the level is still running"); }
    if (!h->base_valid) return fail(h, MPC_ERR_STATE, "no base-set result (mpc_level_start without MPC_LEVEL_THEN_BASE, or the check was left to the caller)");
    if (status) *status = h->base_status;
    if (n_regions) *n_regions = h->base_regions;
    if (h->base_regions > 0) {
        if (rec_d) std::memcpy(rec_d, h->base_rec_d.data(), sizeof(double) * h->base_rec_d.size());
        if (rec_i) std::memcpy(rec_i, h->base_rec_i.data(), sizeof(int32_t) * h->base_rec_i.size());
    }
    h->base_valid = false;
    return MPC_OK;
}

int mpc_level_status(mpc_handle *h, uint8_t *status) {
    if (!h || !status) return MPC_ERR_INVALID;
    if (!h->level_done) return fail(h, MPC_ERR_STATE, "mpc_level_run has not been called for this frontier");
    if (h->n > 0) {
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipMemcpyAsync(status, h->status.p, (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return MPC_OK;
}

#ifdef MPC_XQ_HIST
// debug build only: histogram of k_xq's decisions, [outcome + 1][ratio tests passed]; reset after reading
int mpc_debug_xq_hist(unsigned long long *out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_xq_hist), 64 * sizeof(unsigned long long)) != hipSuccess) return MPC_ERR_HIP;
    if (hipMemcpyFromSymbol(out + 64, HIP_SYMBOL(g_xq_hist2), 64 * sizeof(unsigned long long)) != hipSuccess) return MPC_ERR_HIP;
    unsigned long long z[64] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_xq_hist2), z, sizeof(z)) != hipSuccess) return MPC_ERR_HIP;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_xq_hist), z, sizeof(z)) == hipSuccess ? MPC_OK : MPC_ERR_HIP;
}
#endif
int mpc_engine_kind(mpc_handle *h, int32_t out[8]) {
    if (!h || !out) return MPC_ERR_INVALID;
    const bool fast = h->fast && !h->kn.force_v1;
    out[0] = fast ? 1 : 0;
    out[1] = fast ? (h->fast_t & 1) + 1 : 0;
    out[2] = fast ? (h->fast_x & 1) + 1 : 0;
    out[3] = (fast && h->fast_r >= 0) ? (h->fast_r & 1) + 1 : 0;
    out[4] = fast ? (h->fast_t <= 1 ? 4 : (h->fast_t <= 3 ? 8 : 10)) : 0;
    out[5] = h->theta_open ? 1 : 0;
    out[6] = h->kkt_mode;
    out[7] = (fast && h->kkt_mode == 0 && h->kn.no_kkt_thread != 1) ? KKT_THREAD_MAX : 0;
    return MPC_OK;
}
int mpc_sync(mpc_handle *h) {
    if (!h) return MPC_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (fetch_many_wait(h->device) != MPC_OK) return fail(h, MPC_ERR_HIP, "mpc_sync: the shared record copy (k_fetch_many) failed");   // (its stream may be another member's)
    return MPC_OK;
}

// ---- pooled page-locked host memory (host_pool_* above) ------------------------------------------------------------------
int mpc_host_alloc(uint64_t bytes, void **out) {
    if (!out) return MPC_ERR_INVALID;
    *out = nullptr;
    if (host_pool_take((size_t)bytes, out, nullptr) != hipSuccess) return fail(nullptr, MPC_ERR_HIP, "hipHostMalloc failed");
    return MPC_OK;
}

int mpc_host_free(void *p) {
    if (!p) return MPC_OK;
    return host_pool_give(p) ? MPC_OK : MPC_ERR_INVALID;
}

static int copy_out(mpc_handle *h, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    if (bytes == 0) return MPC_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, kind, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // caller-owned memory: complete before returning
    return MPC_OK;
}

int mpc_level_children(mpc_handle *h, int32_t *out, int64_t cap) {
    if (!h || (!out && cap > 0)) return MPC_ERR_INVALID;
    if (!h->level_done) return fail(h, MPC_ERR_STATE, "mpc_level_run has not been called for this frontier");
    if (cap < h->n_children) return fail(h, MPC_ERR_CAPACITY, "children buffer too small");
    return copy_out(h, out, h->children.p, (size_t)h->n_children * (h->k + 1) * sizeof(int32_t), hipMemcpyDeviceToHost);
}
int mpc_level_children_device(mpc_handle *h, int32_t *out, int64_t cap) {
    if (!h || (!out && cap > 0)) return MPC_ERR_INVALID;
    if (!h->level_done) return fail(h, MPC_ERR_STATE, "mpc_level_run has not been called for this frontier");
    if (cap < h->n_children) return fail(h, MPC_ERR_CAPACITY, "children buffer too small");
    return copy_out(h, out, h->children.p, (size_t)h->n_children * (h->k + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice);
}
int mpc_level_pruned_new(mpc_handle *h, uint64_t *out, int64_t cap) {
    if (!h || (!out && cap > 0)) return MPC_ERR_INVALID;
    if (!h->level_done) return fail(h, MPC_ERR_STATE, "mpc_level_run has not been called for this frontier");
    if (cap < h->n_pruned_new) return fail(h, MPC_ERR_CAPACITY, "pruned buffer too small");
    return copy_out(h, out, h->pruned.as<uint64_t>() + (size_t)h->n_pruned * h->mw, (size_t)h->n_pruned_new * h->mw * sizeof(uint64_t), hipMemcpyDeviceToHost);
}
int mpc_level_pruned_new_device(mpc_handle *h, uint64_t *out, int64_t cap) {
    if (!h || (!out && cap > 0)) return MPC_ERR_INVALID;
    if (!h->level_done) return fail(h, MPC_ERR_STATE, "mpc_level_run has not been called for this frontier");
    if (cap < h->n_pruned_new) return fail(h, MPC_ERR_CAPACITY, "pruned buffer too small");
    return copy_out(h, out, h->pruned.as<uint64_t>() + (size_t)h->n_pruned * h->mw, (size_t)h->n_pruned_new * h->mw * sizeof(uint64_t), hipMemcpyDeviceToDevice);
}

int mpc_frontier_advance(mpc_handle *h) {
    if (!h) return MPC_ERR_INVALID;
    if (!h->level_done) return fail(h, MPC_ERR_STATE, "mpc_level_run has not been called for this frontier");
    h->n_pruned += h->n_pruned_new + h->n_pruned_extra;   // already in place behind the list (no copy)
    h->n_pruned_extra = 0;
    std::swap(h->frontier, h->children);
    std::swap(h->parent_slot, h->parent_slot_next);
    h->have_parent_slot = true;
    h->have_prev_dict = h->storing;
    h->dict_cur = 1 - h->dict_cur;
    h->storing = false;
    h->prev_regions = h->n_regions;
    h->n_prev = h->n;   // the frontier that has just been left sits in h->children until this level writes its own children
    h->n = h->n_children;
    h->k = h->k + 1;
    h->level_done = false;
    h->n_children = 0; h->n_pruned_new = 0; h->n_regions = 0; h->n_opt = 0;
    return MPC_OK;
}
int mpc_frontier_advance_batch(mpc_handle **hs, int32_t n_handles) {
    if (!hs || n_handles < 0) return MPC_ERR_INVALID;
    for (int i = 0; i < n_handles; ++i) { const int rc = mpc_frontier_advance(hs[i]); if (rc != MPC_OK) return rc; }
    return MPC_OK;
}

// ---- the level loop of many programs on a thread of the library (include/mpcombi.h: mpc_solve_many_*) ----------------------------------
struct ManyLevel {
    std::vector<int32_t> member;
    std::vector<mpc_level_stats> stats;
    std::vector<int64_t> ns, nr, od, oi, oe;
    void *hd = nullptr, *hi = nullptr, *er = nullptr;
    int64_t ld = 0, li = 0, le = 0;
    int32_t n_shared = 0;
    double ms_wall = 0;
    bool base = false;       // the closing level of the base active sets
    bool taken = false;      // the blocks belong to the caller
    ~ManyLevel() { if (!taken) { if (hd) (void)host_pool_give(hd); if (hi) (void)host_pool_give(hi); if (er) (void)host_pool_give(er); } }
};
struct ManyJob {
    std::vector<mpc_handle *> hs;
    std::vector<int32_t> max_levels;
    int32_t flags = 0;
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::vector<std::unique_ptr<ManyLevel>> levels;   // appended by the loop, read by the caller (under m)
    bool finished = false, handover = false;
    int rc = MPC_OK;
};

static void many_loop(ManyJob *J) {
    auto finish = [&](int rc) {
        std::lock_guard<std::mutex> lk(J->m);
        J->rc = rc; J->finished = true;
        J->cv.notify_all();
    };
    const int B = (int)J->hs.size();
    if (B == 0) return finish(MPC_OK);
    mpc_handle *h0 = J->hs[0];
    if (hipSetDevice(h0->device) != hipSuccess) return finish(fail(h0, MPC_ERR_HIP, "mpc_solve_many: hipSetDevice failed"));
    const double budget_gb = 0.6 * batch_budget_gb();   // (headroom as in the host layer's loop)
    std::vector<int> depth(B, 0);
    std::vector<int32_t> active;
    for (int i = 0; i < B; ++i) {
        mpc_handle *h = J->hs[i];
        int rc = mpc_pruned_clear(h);
        if (rc == MPC_OK) rc = mpc_frontier_root(h);
        if (rc != MPC_OK) return finish(rc);
        if (J->max_levels[i] > 0) active.push_back(i);
    }
    auto gen_of = [&](int i) { return depth[i] + 1 != J->max_levels[i] ? 1 : 0; };
    auto start = [&](const std::vector<int32_t> &act, void **token) -> int {
        std::vector<mpc_handle *> hh; std::vector<int32_t> gg;
        for (int i : act) { hh.push_back(J->hs[i]); gg.push_back(gen_of(i)); }
        return mpc_level_batch_start(hh.data(), (int32_t)hh.size(), gg.data(), J->flags & ~MPC_SOLVE_MANY_BASE, token);
    };
    void *token = nullptr;
    const bool dbg = debug_many();
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms_since = [&](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(now() - a).count(); };
    { const auto ts = now(); if (!active.empty()) { const int rc = start(active, &token); if (rc != MPC_OK) return finish(rc); } if (dbg) std::fprintf(stderr, "[many] first start %.3f ms\n", ms_since(ts)); }
    bool base_phase = false;
    auto start_base = [&]() -> int {      // every program's base active set as one more shared level (reference driver :142-146)
        active.clear();
        for (int i = 0; i < B; ++i) {
            mpc_handle *h = J->hs[i];
            int rc = frontier_reset(h, 1, h->n_eq);
            if (rc != MPC_OK) return rc;
            if (h->n_eq > 0) { hipLaunchKernelGGL(k_base_frontier, dim3(1), dim3(64), 0, h->stream, h->n_eq, h->frontier.as<int32_t>()); HIP_TRY(h, hipGetLastError()); }
            h->n_pruned = 0; h->n_pruned_extra = 0;
            active.push_back(i);
        }
        for (int i = 0; i < B; ++i) if (J->hs[i]->stream != J->hs[0]->stream && J->hs[i]->n_eq > 0) HIP_TRY(J->hs[i], hipStreamSynchronize(J->hs[i]->stream));   // (the shared launches run on the first member's stream)
        base_phase = true;
        std::vector<mpc_handle *> hh(J->hs); std::vector<int32_t> gg(B, 0);
        return mpc_level_batch_start(hh.data(), B, gg.data(), J->flags & ~MPC_SOLVE_MANY_BASE, &token);
    };
    if (active.empty() && (J->flags & MPC_SOLVE_MANY_BASE)) { const int rc = start_base(); if (rc != MPC_OK) return finish(rc); }
    while (!active.empty()) {
        const auto t0 = std::chrono::steady_clock::now();
        double t_wait = 0, t_fetch = 0, t_adv = 0, t_start = 0;
        const int nb = (int)active.size();
        std::unique_ptr<ManyLevel> L(new ManyLevel());
        L->member = active;
        L->base = base_phase;
        L->stats.resize(nb);
        {
            // (mpc_level_batch_wait writes stats[m.id] with ids = positions in ITS handle list = positions in `active`)
            const auto ts = now();
            const int rc = mpc_level_batch_wait(token, L->stats.data(), &L->n_shared);
            t_wait = ms_since(ts);
            token = nullptr;
            if (rc != MPC_OK) return finish(rc);
        }
        // the level's records: three blocks for all members (sizes from each member's statistics, as the host layer's level_batch_fetch)
        const auto tf = now();
        L->ns.assign(nb, 0); L->nr.assign(nb, 0); L->od.assign(nb, 0); L->oi.assign(nb, 0); L->oe.assign(nb, 0);
        std::vector<int64_t> fds(nb), fis(nb);
        for (int j = 0; j < nb; ++j) {
            const mpc_handle *h = J->hs[active[j]];
            const RecordSizes z = level_record_sizes(h, L->stats[j]);
            fds[j] = z.fd; fis[j] = z.fi; L->ns[j] = z.n_slots; L->nr[j] = z.rows_cap;
            L->od[j] = L->ld; L->oi[j] = L->li; L->oe[j] = L->le;
            L->ld += L->ns[j] * fds[j]; L->li += L->ns[j] * fis[j]; L->le += L->nr[j] * (h->n_t + 1);
        }
        if (L->ld > 0) {
            if (host_pool_take((size_t)L->ld * 8, &L->hd, nullptr) != hipSuccess || host_pool_take((size_t)L->li * 4, &L->hi, nullptr) != hipSuccess ||
                host_pool_take((size_t)std::max<int64_t>(L->le, 1) * 8, &L->er, nullptr) != hipSuccess)
                return finish(fail(h0, MPC_ERR_HIP, "mpc_solve_many: page-locked memory for the level's records"));
            std::vector<mpc_handle *> hh; std::vector<double *> pd, pe; std::vector<int32_t *> pi; std::vector<int64_t> cs, cr, n1, n2; std::vector<int> at;
            for (int j = 0; j < nb; ++j) {
                if (L->ns[j] == 0) continue;
                hh.push_back(J->hs[active[j]]); at.push_back(j);
                pd.push_back(static_cast<double *>(L->hd) + L->od[j]); pi.push_back(static_cast<int32_t *>(L->hi) + L->oi[j]);
                pe.push_back(static_cast<double *>(L->er) + L->oe[j]);
                cs.push_back(L->ns[j]); cr.push_back(L->nr[j]);
            }
            n1.assign(hh.size(), 0); n2.assign(hh.size(), 0);
            const int rc = mpc_level_batch_fetch(hh.data(), (int32_t)hh.size(), pd.data(), pi.data(), cs.data(), pe.data(), cr.data(), n1.data(), n2.data());
            if (rc != MPC_OK) return finish(rc);
            for (size_t q = 0; q < hh.size(); ++q) { L->ns[at[q]] = n1[q]; L->nr[at[q]] = n2[q]; }
            // a member outside the shared copy launch (records re-solved by the LDS engine, streamed ...) queued its copies on its own stream
            for (mpc_handle *h : hh) if (hipStreamQuery(h->stream) != hipSuccess) { (void)hipGetLastError(); if (hipStreamSynchronize(h->stream) != hipSuccess) return finish(fail(h, MPC_ERR_HIP, "mpc_solve_many: record copy")); }
        }
        t_fetch = ms_since(tf);
        const auto ta = now();
        std::vector<int32_t> nxt;
        if (!base_phase) for (int j = 0; j < nb; ++j) if (gen_of(active[j]) && L->stats[j].n_children > 0) nxt.push_back(active[j]);
        double need_gb = 0.0;
        for (int i : nxt) {
            const int rc = mpc_frontier_advance(J->hs[i]);
            if (rc != MPC_OK) return finish(rc);
            depth[i] += 1;
            need_gb += batch_level_gb(J->hs[i], gen_of(i));
        }
        const bool handover = !nxt.empty() && need_gb > budget_gb;
        t_adv = ms_since(ta);
        const auto tst = now();
        const bool then_base = nxt.empty() && !base_phase && (J->flags & MPC_SOLVE_MANY_BASE);
        if (!nxt.empty() && !handover) {
            const int rc = start(nxt, &token);      // (waits for the shared record copy first: the members' record buffers are written again)
            if (rc != MPC_OK) return finish(rc);
        } else if (then_base) {
            const int rc = start_base();
            if (rc != MPC_OK) return finish(rc);
        } else if (fetch_many_wait(h0->device) != MPC_OK) return finish(fail(h0, MPC_ERR_HIP, "mpc_solve_many: the shared record copy failed"));
        t_start = ms_since(tst);
        L->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (dbg) std::fprintf(stderr, "[many] level of %d members: wait+finish %.3f fetch %.3f advance %.3f next start %.3f total %.3f ms\n", nb, t_wait, t_fetch, t_adv, t_start, L->ms_wall);
        {
            std::lock_guard<std::mutex> lk(J->m);
            J->levels.push_back(std::move(L));
            if (handover) J->handover = true;
            J->cv.notify_all();
        }
        if (handover) break;
        if (then_base) continue;      // (`active` = every member, set by start_base)
        active.swap(nxt);
    }
    finish(MPC_OK);
}

extern "C" int mpc_solve_many_start(mpc_handle **hs, int32_t n_handles, const int32_t *max_levels, int32_t flags, void **job) {
    if (!hs || n_handles < 0 || !max_levels || !job) return MPC_ERR_INVALID;
    *job = nullptr;
    for (int i = 0; i < n_handles; ++i) {
        if (!hs[i]) return MPC_ERR_INVALID;
        std::lock_guard<std::mutex> lk(hs[i]->wm);
        if (hs[i]->w_busy) return fail(hs[i], MPC_ERR_STATE, "a level started with mpc_level_start is still running");
    }
    std::unique_ptr<ManyJob> J(new ManyJob());
    J->hs.assign(hs, hs + n_handles);
    J->max_levels.assign(max_levels, max_levels + n_handles);
    J->flags = flags & (MPC_LEVEL_KEEP_LOWDIM | MPC_SOLVE_MANY_BASE);
    ManyJob *raw = J.get();
    try { J->th = std::thread(many_loop, raw); } catch (...) { return fail(n_handles ? hs[0] : nullptr, MPC_ERR_STATE, "mpc_solve_many_start: no thread"); }
    *job = J.release();
    return MPC_OK;
}
extern "C" int mpc_solve_many_level(void *job, int32_t level, mpc_many_level_info *info) {
    if (!job || !info || level < 0) return MPC_ERR_INVALID;
    ManyJob *J = static_cast<ManyJob *>(job);
    std::unique_lock<std::mutex> lk(J->m);
    J->cv.wait(lk, [&] { return (int)J->levels.size() > level || J->finished; });
    std::memset(info, 0, sizeof(*info));
    info->level = level;
    if ((int)J->levels.size() <= level) {
        info->done = J->handover ? 2 : 1;
        return J->rc;
    }
    ManyLevel &L = *J->levels[level];
    info->n_members = (int32_t)L.member.size(); info->n_shared = L.n_shared; info->base = L.base ? 1 : 0;
    info->member = L.member.data(); info->stats = L.stats.data();
    info->n_slots = L.ns.data(); info->n_rows = L.nr.data(); info->off_d = L.od.data(); info->off_i = L.oi.data(); info->off_e = L.oe.data();
    info->head_d = static_cast<double *>(L.hd); info->head_i = static_cast<int32_t *>(L.hi); info->erows = static_cast<double *>(L.er);
    info->len_d = L.ld; info->len_i = L.li; info->len_e = std::max<int64_t>(L.le, L.hd ? 1 : 0);
    info->ms_wall = L.ms_wall;
    L.taken = true;
    return MPC_OK;
}
extern "C" int mpc_solve_many_wait(void *job) {
    if (!job) return MPC_ERR_INVALID;
    std::unique_ptr<ManyJob> J(static_cast<ManyJob *>(job));
    if (J->th.joinable()) J->th.join();
    return J->rc;
}

}  // extern "C"

// ---- connected-graph traversal, bookkeeping on the device (graph.hpp) ---------------------------------------------------------
namespace {
struct GDec2 { __host__ __device__ rocprim::tuple<unsigned long long &, unsigned long long &> operator()(GMask<2> &k) const {
    return rocprim::tuple<unsigned long long &, unsigned long long &>(k.w[1], k.w[0]); } };
struct GDec4 { __host__ __device__ rocprim::tuple<unsigned long long &, unsigned long long &, unsigned long long &, unsigned long long &> operator()(GMask<4> &k) const {
    return rocprim::tuple<unsigned long long &, unsigned long long &, unsigned long long &, unsigned long long &>(k.w[3], k.w[2], k.w[1], k.w[0]); } };
template <int MW> struct GDec;
template <> struct GDec<2> { typedef GDec2 type; };
template <> struct GDec<4> { typedef GDec4 type; };
constexpr long long G_CHUNK = 1ll << 22;   // masks per group run (bounds the level buffers and the 32-bit neighbour offsets)

template <int MW>
int g_sort(mpc_handle *h, const GMask<MW> *in, GMask<MW> *out, long long n) {
    if (n <= 0) return MPC_OK;
    size_t bytes = 0;
    typename GDec<MW>::type dec;
    HIP_TRY(h, rocprim::radix_sort_keys(nullptr, bytes, const_cast<GMask<MW> *>(in), out, (size_t)n, dec, 0u, 64u * MW, h->stream));
    HIP_TRY(h, h->g.sort_tmp.ensure(std::max<size_t>(bytes, 16), h->stream));
    bytes = h->g.sort_tmp.cap;
    HIP_TRY(h, rocprim::radix_sort_keys(h->g.sort_tmp.p, bytes, const_cast<GMask<MW> *>(in), out, (size_t)n, dec, 0u, 64u * MW, h->stream));
    return MPC_OK;
}

// pending (n_pending masks, any order, duplicates) -> next wave (sorted by cardinality, then mask) and visited := visited + new
template <int MW>
int g_close(mpc_handle *h) {
    auto &g = h->g;
    hipStream_t st = h->stream;
    const long long n = g.n_pending;
    g.gk.clear(); g.goff.clear(); g.gcnt.clear();
    g.n_wave = 0;
    g.n_pending = 0;
    if (n == 0) return MPC_OK;
    typedef GMask<MW> M;
    const unsigned nb = (unsigned)((n + 255) / 256);
    HIP_TRY(h, g.tmp_a.ensure((size_t)n * sizeof(M), st));
    { int rc = g_sort<MW>(h, g.pending.as<M>(), g.tmp_a.as<M>(), n); if (rc) return rc; }
    HIP_TRY(h, h->flag.ensure((size_t)n * sizeof(int32_t), st));
    HIP_TRY(h, h->pos.ensure((size_t)n * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_g_newflags<MW>, dim3(nb), dim3(256), 0, st, g.tmp_a.as<M>(), n, g.visited.as<M>(), g.n_visited, h->flag.as<int32_t>());
    { int rc = launch_scan(h, h->flag.as<int32_t>(), h->pos.as<int32_t>(), n, h->tot_dev); if (rc) return rc; }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(st));
    const long long n_new = h->tot_host[0];
    if (n_new == 0) return MPC_OK;
    // visited ++ new, sorted
    HIP_TRY(h, g.tmp_b.ensure((size_t)(g.n_visited + n_new) * sizeof(M), st));
    if (g.n_visited > 0) HIP_TRY(h, hipMemcpyAsync(g.tmp_b.p, g.visited.p, (size_t)g.n_visited * sizeof(M), hipMemcpyDeviceToDevice, st));
    M *fresh = g.tmp_b.as<M>() + g.n_visited;   // the new masks, sorted by mask
    hipLaunchKernelGGL(k_g_compact<MW>, dim3(nb), dim3(256), 0, st, g.tmp_a.as<M>(), n, h->flag.as<int32_t>(), h->pos.as<int32_t>(), fresh);
    HIP_TRY(h, hipGetLastError());
    // next wave: the new masks in (cardinality, mask) order -- a stable sort of their cardinalities carries the permutation
    const unsigned nbn = (unsigned)((n_new + 255) / 256);
    for (DevBuf *b : {&g.card, &g.idx, &g.card2, &g.idx2}) HIP_TRY(h, b->ensure((size_t)n_new * sizeof(unsigned int), st));
    hipLaunchKernelGGL(k_g_card<MW>, dim3(nbn), dim3(256), 0, st, fresh, n_new, g.card.as<unsigned int>(), g.idx.as<unsigned int>());
    {
        size_t bytes = 0;
        HIP_TRY(h, rocprim::radix_sort_pairs(nullptr, bytes, g.card.as<unsigned int>(), g.card2.as<unsigned int>(), g.idx.as<unsigned int>(), g.idx2.as<unsigned int>(),
                                             (size_t)n_new, 0u, 9u, st));
        HIP_TRY(h, g.sort_tmp.ensure(std::max<size_t>(bytes, 16), st));
        bytes = g.sort_tmp.cap;
        HIP_TRY(h, rocprim::radix_sort_pairs(g.sort_tmp.p, bytes, g.card.as<unsigned int>(), g.card2.as<unsigned int>(), g.idx.as<unsigned int>(), g.idx2.as<unsigned int>(),
                                             (size_t)n_new, 0u, 9u, st));
    }
    HIP_TRY(h, g.wave.ensure((size_t)n_new * sizeof(M), st));
    hipLaunchKernelGGL(k_g_gather<MW>, dim3(nbn), dim3(256), 0, st, fresh, g.idx2.as<unsigned int>(), n_new, g.wave.as<M>());
    HIP_TRY(h, g.hist.ensure(257 * sizeof(int32_t), st));
    HIP_TRY(h, hipMemsetAsync(g.hist.p, 0xff, 257 * sizeof(int32_t), st));   // -1: no mask of that cardinality
    hipLaunchKernelGGL(k_g_first, dim3(nbn), dim3(256), 0, st, g.card2.as<unsigned int>(), n_new, g.hist.as<int32_t>());
    HIP_TRY(h, hipGetLastError());
    int32_t hist[257];
    HIP_TRY(h, hipMemcpyAsync(hist, g.hist.p, sizeof(hist), hipMemcpyDeviceToHost, st));
    // visited := sort(visited ++ new)   (tmp_b -> visited)
    HIP_TRY(h, g.visited.ensure((size_t)(g.n_visited + n_new) * sizeof(M), st));
    { int rc = g_sort<MW>(h, g.tmp_b.as<M>(), g.visited.as<M>(), g.n_visited + n_new); if (rc) return rc; }
    HIP_TRY(h, hipStreamSynchronize(st));
    g.n_visited += n_new;
    g.n_wave = n_new;
    // hist[k] = index of the first mask with k rows (-1: none); a group ends where the next present cardinality starts
    long long end = n_new;
    std::vector<std::pair<int, std::pair<long long, long long>>> groups;   // (k, (first, count)), built from the back
    for (int k = 256; k >= 0; --k) {
        if (hist[k] < 0) continue;
        groups.push_back({k, {hist[k], end - hist[k]}});
        end = hist[k];
    }
    for (auto it = groups.rbegin(); it != groups.rend(); ++it) {
        long long off = it->second.first, c = it->second.second;
        while (c > 0) { const long long take = std::min(c, G_CHUNK); g.gk.push_back(it->first); g.goff.push_back(off); g.gcnt.push_back(take); off += take; c -= take; }
    }
    return MPC_OK;
}

template <int MW>
int g_group_run(mpc_handle *h, int gi, mpc_level_stats *stats) {
    auto &g = h->g;
    typedef GMask<MW> M;
    hipStream_t st = h->stream;
    const int k = g.gk[gi];
    const long long off = g.goff[gi], cnt = g.gcnt[gi];
    const M *masks = g.wave.as<M>() + off;
    const unsigned nb = (unsigned)((cnt + 255) / 256);
    const bool too_many_rows = k > std::min(h->n_x, h->n_c);   // more rows than variables: rank deficient by counting (is_full_rank)
    mpc_level_stats ls;
    std::memset(&ls, 0, sizeof(ls));
    ls.n = cnt; ls.k = k;
    if (too_many_rows) ls.n_status[ST_INFEASIBLE] = cnt;
    else {
        int rc = frontier_reset(h, cnt, k);
        if (rc) return rc;
        if (k > 0) hipLaunchKernelGGL(k_g_frontier<MW>, dim3(nb), dim3(256), 0, st, masks, cnt, k, h->frontier.as<int32_t>());
        HIP_TRY(h, hipGetLastError());
        // Both traversals only need "rank deficient / no region / non-empty but lower dimensional / region": mpqp_graph.py hands on
        // the same subsets whether a set is infeasible or feasible but not optimal (:69-91; only its pruning list tells them apart,
        // and no pruning list is kept here), so the (x,theta) feasibility LP is left out for it as well.
        rc = level_run_impl(h, 0, MPC_LEVEL_GRAPH, &ls);
        if (rc) return rc;
    }
    if (stats) *stats = ls;
    // facet constraints of the regions (variant 1)
    const M *facet = nullptr;
    if (g.variant == 1 && !too_many_rows && ls.n_regions > 0) {
        HIP_TRY(h, g.facet.ensure((size_t)cnt * sizeof(M), st));
        HIP_TRY(h, hipMemsetAsync(g.facet.p, 0, (size_t)cnt * sizeof(M), st));
        if (h->used_region2 && h->n_opt > 0)
            hipLaunchKernelGGL(k_g_facets_slots<MW>, dim3((unsigned)((h->n_opt + 255) / 256)), dim3(256), 0, st, h->headi.as<int32_t>(), h->fi, h->n_opt, k, h->n_c,
                               h->n_tc, g.facet.as<M>());
        const int32_t *list = h->used_region2 ? h->retry_list.as<int32_t>() : h->opt_ptr;
        const long long n_list = h->used_region2 ? h->n_rretry : h->n_opt;
        if (n_list > 0)
            hipLaunchKernelGGL(k_g_facets_fixed<MW>, dim3((unsigned)((n_list + 255) / 256)), dim3(256), 0, st, h->reci.as<int32_t>(), h->rec_i, list, n_list,
                               h->status.as<uint8_t>(), h->n_c, h->n_tc, g.facet.as<M>());
        HIP_TRY(h, hipGetLastError());
        facet = g.facet.as<M>();
    } else if (g.variant == 1) {
        HIP_TRY(h, g.facet.ensure((size_t)cnt * sizeof(M), st));
        HIP_TRY(h, hipMemsetAsync(g.facet.p, 0, (size_t)cnt * sizeof(M), st));
        facet = g.facet.as<M>();
    }
    // neighbours: count -> scan -> emit behind what the earlier groups of this wave have emitted
    M eq, all;
    for (int j = 0; j < MW; ++j) { eq.w[j] = 0; all.w[j] = 0; }
    for (int i = 0; i < h->n_eq; ++i) eq.w[i >> 6] |= 1ull << (i & 63);
    for (int i = 0; i < h->n_c; ++i) all.w[i >> 6] |= 1ull << (i & 63);
    const uint8_t *status = too_many_rows ? nullptr : h->status.as<uint8_t>();
    HIP_TRY(h, g.cnt.ensure((size_t)cnt * sizeof(int32_t), st));
    HIP_TRY(h, g.off.ensure((size_t)cnt * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_g_count<MW>, dim3(nb), dim3(256), 0, st, masks, cnt, status, (int)ST_INFEASIBLE, g.variant, eq, all, facet, g.cnt.as<int32_t>());
    { int rc = launch_scan(h, g.cnt.as<int32_t>(), g.off.as<int32_t>(), cnt, h->tot_dev); if (rc) return rc; }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(st));
    const long long total = h->tot_host[0];
    if (total > 0) {
        HIP_TRY(h, g.pending.ensure((size_t)(g.n_pending + total) * sizeof(M), st, true));
        hipLaunchKernelGGL(k_g_emit<MW>, dim3(nb), dim3(256), 0, st, masks, cnt, status, (int)ST_INFEASIBLE, g.variant, eq, all, facet, g.off.as<int32_t>(),
                           g.pending.as<M>() + g.n_pending);
        HIP_TRY(h, hipGetLastError());
        g.n_pending += total;
    }
    return MPC_OK;
}
}  // namespace

extern "C" {

int mpc_graph_begin(mpc_handle *h, const uint64_t *seed_masks, int64_t n_seeds, int32_t variant) {
    if (!h || (n_seeds > 0 && !seed_masks) || n_seeds < 0 || variant < 0 || variant > 1) return MPC_ERR_INVALID;
    { std::lock_guard<std::mutex> lk(h->wm); if (h->w_busy) return fail(h, MPC_ERR_STATE, "a level started with mpc_level_start is still running"); }
    HIP_TRY(h, hipSetDevice(h->device));
    auto &g = h->g;
    g.active = true; g.variant = variant; g.n_wave = g.n_visited = 0; g.n_pending = n_seeds;
    if (n_seeds > 0) {
        HIP_TRY(h, g.pending.ensure((size_t)n_seeds * h->mw * sizeof(uint64_t), h->stream));
        HIP_TRY(h, hipMemcpyAsync(g.pending.p, seed_masks, (size_t)n_seeds * h->mw * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return h->mw == 2 ? g_close<2>(h) : g_close<4>(h);
}

int mpc_graph_wave(mpc_handle *h, int32_t *k_list, int64_t *count_list, int32_t cap, int32_t *n_groups, int64_t *n_wave, int64_t *n_visited) {
    if (!h || !n_groups) return MPC_ERR_INVALID;
    if (!h->g.active) return fail(h, MPC_ERR_STATE, "mpc_graph_begin has not been called");
    const int ng = (int)h->g.gk.size();
    *n_groups = ng;
    if (n_wave) *n_wave = h->g.n_wave;
    if (n_visited) *n_visited = h->g.n_visited;
    if (cap < ng) return ng == 0 ? MPC_OK : fail(h, MPC_ERR_CAPACITY, "group arrays too small");
    for (int i = 0; i < ng; ++i) { if (k_list) k_list[i] = h->g.gk[i]; if (count_list) count_list[i] = h->g.gcnt[i]; }
    return MPC_OK;
}

int mpc_graph_group_run(mpc_handle *h, int32_t group, mpc_level_stats *stats) {
    if (!h) return MPC_ERR_INVALID;
    if (!h->g.active || group < 0 || group >= (int)h->g.gk.size()) return fail(h, MPC_ERR_STATE, "no such group in the current wave");
    { std::lock_guard<std::mutex> lk(h->wm); if (h->w_busy) return fail(h, MPC_ERR_STATE, "a level started with mpc_level_start is still running"); }
    HIP_TRY(h, hipSetDevice(h->device));
    return h->mw == 2 ? g_group_run<2>(h, group, stats) : g_group_run<4>(h, group, stats);
}

int mpc_graph_wave_close(mpc_handle *h, int64_t *n_next, int64_t *n_visited) {
    if (!h) return MPC_ERR_INVALID;
    if (!h->g.active) return fail(h, MPC_ERR_STATE, "mpc_graph_begin has not been called");
    HIP_TRY(h, hipSetDevice(h->device));
    const int rc = h->mw == 2 ? g_close<2>(h) : g_close<4>(h);
    if (n_next) *n_next = h->g.n_wave;
    if (n_visited) *n_visited = h->g.n_visited;
    return rc;
}

int mpc_check_level(mpc_handle *h, const int32_t *cand, int64_t n, int32_t k, const uint64_t *pruned_masks, int64_t m,
                    int32_t gen_children, uint8_t *status, int64_t *n_regions, double *rec_d, int32_t *rec_i,
                    int64_t *region_cand, int64_t region_cap, int64_t *n_children, int32_t *children, int64_t children_cap) {
    if (!h) return MPC_ERR_INVALID;
    int rc = mpc_frontier_set(h, cand, n, k);
    if (rc) return rc;
    mpc_pruned_clear(h);
    rc = mpc_pruned_add(h, pruned_masks, m);
    if (rc) return rc;
    mpc_level_stats stats;
    rc = mpc_level_run(h, gen_children, &stats);
    if (rc) return rc;
    if (status) { rc = mpc_level_status(h, status); if (rc) return rc; }
    if (n_regions) *n_regions = stats.n_regions;
    if (n_children) *n_children = stats.n_children;
    if (stats.n_regions > region_cap || stats.n_children > children_cap) return fail(h, MPC_ERR_CAPACITY, "output buffers too small");
    if (stats.n_regions > 0) { rc = mpc_level_regions(h, rec_d, rec_i, region_cand, region_cap); if (rc) return rc; }
    if (stats.n_children > 0) { rc = mpc_level_children(h, children, children_cap); if (rc) return rc; }
    return MPC_OK;
}

}  // extern "C"

// ---- the QP of the program at fixed parameter points (qp_batch of points.hip) ---------------------------------------------------
extern "C" int mpc_qp_solve_batch(mpc_handle *h, int64_t m, const double *theta, int32_t *status, double *x, double *lambda, uint8_t *active,
                                  int32_t *iters) {
    if (!h || m < 0 || (m > 0 && (!theta || !status))) return MPC_ERR_INVALID;
    if (!h->is_qp || h->kkt_mode != 0) return fail(h, MPC_ERR_INVALID, "mpc_qp_solve_batch needs a positive definite Q");
    if (m == 0) return MPC_OK;
    { std::lock_guard<std::mutex> lk(h->wm); if (h->w_busy) return fail(h, MPC_ERR_STATE, "a level started with mpc_level_start is still running"); }
    HIP_TRY(h, hipSetDevice(h->device));
    return qp_batch(h, h->stream, h->n_cu, QpProgram{h->n_c, h->n_eq, h->n_t, h->n_x, h->Pv.W, h->Pv.UV, h->Pv.X0H, h->Pv.Gt}, m, theta, status, x, lambda,
                    active, iters);
}
