// host_common.hpp -- what the host code of mpcombi_hip.hip (the engine), geometry.hip and points.hip shares: the process-wide pools
// of device blocks, pinned host blocks, streams and events, the error channel, the scaffold of a one-shot call (OneShot), and the two
// calls of points.hip that the engine makes.
//
// Host code only; no kernels.  The pool state itself (mutexes, free maps, the thread-local error string, the CU-count cache) is
// defined exactly once, in mpcombi_hip.hip: every unit recycles the same blocks, streams and events.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <deque>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mpcombi.h"

namespace mpc {

// ---- process-wide recycling (definitions and the story: mpcombi_hip.hip) --------------------------------------------------------
size_t dev_size_class(size_t bytes);
hipError_t dev_pool_take(size_t cls, void **out);
void dev_pool_give(void *p, size_t cls);
hipError_t host_pool_take(size_t bytes, void **out, size_t *got, bool coherent = false);
bool host_pool_give(void *p);
hipError_t pooled_stream(hipStream_t *out);
void return_stream(hipStream_t s);   // synchronised by the caller
hipError_t pooled_event(hipEvent_t *out, bool timing);
void return_event(hipEvent_t e, bool timing);
int device_count_cached();
int cu_count(int device);

inline int odd_at_least(int v) { return (v % 2) ? v : v + 1; }
inline int waves_per_cu(int lds_bytes) { return std::max(1, std::min(16, (160 * 1024) / std::max(lds_bytes, 1))); }

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    // != nullptr: a block this buffer has outgrown is parked there instead of being waited for -- the owner (a handle) gives the parked
    // blocks back to the pool behind its next synchronisation of all its streams (graveyard_flush).  A handle's first solve grows some
    // twenty buffers on every level: one stream synchronisation each (round 4: 170 growths per first solve of config 4).
    std::vector<std::pair<void *, size_t>> *parked = nullptr;
    hipError_t ensure(size_t bytes, hipStream_t st, bool keep = false) {
        if (bytes <= cap) return hipSuccess;
        const size_t want = dev_size_class(std::max(bytes, cap + cap / 2));
        void *q = nullptr;
        hipError_t e = dev_pool_take(want, &q);
        if (e != hipSuccess) return e;
        if (p) {
            if (keep && cap) {
                e = hipMemcpyAsync(q, p, cap, hipMemcpyDeviceToDevice, st);
                if (e != hipSuccess) return e;
            }
            // the old block may still be read by work queued on this stream: it goes back to the pool only afterwards
            if (parked) parked->emplace_back(p, cap);
            else {
                e = st ? hipStreamSynchronize(st) : hipDeviceSynchronize();
                if (e != hipSuccess) return e;
                dev_pool_give(p, cap);
            }
        }
        p = q;
        cap = want;
        return hipSuccess;
    }
    // the caller has synchronised whatever used the block
    void release() { if (p) dev_pool_give(p, cap); p = nullptr; cap = 0; }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// pinned (page-locked) host staging: device-to-host copies run at link speed and never page-fault
struct HostBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool coherent = false;   // class 1 of the pool: written by running kernels, polled by the host
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        const size_t want = std::max(bytes, cap + cap / 2);
        release();
        return host_pool_take(want, &p, &cap, coherent);
    }
    void release() { if (p) (void)host_pool_give(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

}  // namespace mpc

// ---- errors -----------------------------------------------------------------------------------------------------------------------
struct mpc_handle;

namespace mpc {

// stores msg as the handle's last error (h == nullptr: the calling thread's global error, mpc_last_global_error) and returns code
int fail(mpc_handle *h, int code, const std::string &msg);

#define HIP_TRY(h, expr)                                                                                   \
    do {                                                                                                   \
        hipError_t e__ = (expr);                                                                           \
        if (e__ != hipSuccess)                                                                             \
            return fail(h, MPC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));               \
    } while (0)

// makes `device` the calling thread's device; who != nullptr prefixes the out-of-range message ("<who>: ...")
inline int select_device(const char *who, int32_t device) {
    const int ndev = device_count_cached();
    if (ndev < 1) return fail(nullptr, MPC_ERR_HIP, "no HIP device available (libmpcombi_hip has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, MPC_ERR_INVALID, std::string(who ? who : "") + (who ? ": " : "") + "device index out of range");
    HIP_TRY(nullptr, hipSetDevice(device));
    return MPC_OK;
}

// ---- one call's device buffers and timing events ------------------------------------------------------------------------------------
// The stateless entry points (a batch in, one or a few launches, the results out) all need the same things: pooled device buffers
// that go back to the pool on every way out, the first HIP error of the call, and sometimes the time between two events around
// the launch.  OneShot owns them.  Its error is sticky: once a step has failed, buffers, copies and launches become no-ops, so the
// steps can be written one after the other; a caller looks at ok() only before the HOST reads what a download brought.
// stream == nullptr: the default stream with blocking copies and hipDeviceSynchronize at the end; otherwise asynchronous copies
// on that stream and hipStreamSynchronize.  OwnStream: a stream of the pool, taken for this call and returned behind its last
// wait -- callers on other threads / handles keep running (no device-wide synchronisation).
struct OneShot {
    struct OwnStream {};
    const char *who;   // the entry point: the error text is "<who>: <hipGetErrorString>"
    hipStream_t st;
    hipEvent_t e0 = nullptr, e1 = nullptr;   // timed: around launch_timed
    hipError_t err = hipSuccess;
    std::deque<DevBuf> bufs;   // a deque: references handed out stay valid
    bool open = true, synced = false, own = false;

    explicit OneShot(const char *who_, hipStream_t st_ = nullptr, bool timed = false) : who(who_), st(st_) {
        if (timed) { chk(hipEventCreate(&e0)); chk(hipEventCreate(&e1)); }
    }
    OneShot(const char *who_, OwnStream) : who(who_), st(nullptr), own(true) { chk(pooled_stream(&st)); }
    OneShot(const OneShot &) = delete;
    OneShot &operator=(const OneShot &) = delete;
    ~OneShot() { close(); }

    bool ok() const { return err == hipSuccess; }
    bool chk(hipError_t e) { if (err == hipSuccess && e != hipSuccess) err = e; return e == hipSuccess; }

    // a buffer of at least `bytes` (0: empty, sized later by ensure / upload)
    DevBuf &buf(size_t bytes = 0) { bufs.emplace_back(); ensure(bufs.back(), bytes); return bufs.back(); }
    void ensure(DevBuf &b, size_t bytes) { if (ok()) chk(b.ensure(bytes, st)); }
    // host -> device into b, grown to max(8, bytes); nothing is copied when bytes == 0
    void upload(DevBuf &b, const void *src, size_t bytes) {
        ensure(b, std::max<size_t>(8, bytes));
        if (ok() && bytes) chk(st ? hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st) : hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    }
    DevBuf &upload(const void *src, size_t bytes) { DevBuf &b = buf(); upload(b, src, bytes); return b; }
    void download(void *dst, const DevBuf &b, size_t bytes) {
        if (ok() && bytes) chk(st ? hipMemcpyAsync(dst, b.p, bytes, hipMemcpyDeviceToHost, st) : hipMemcpy(dst, b.p, bytes, hipMemcpyDeviceToHost));
    }
    void fill(DevBuf &b, int byte, size_t bytes) { if (ok()) chk(st ? hipMemsetAsync(b.p, byte, bytes, st) : hipMemset(b.p, byte, bytes)); }
    // f() enqueues kernels; launch_timed puts the two events around them
    template <class F> void launch(F &&f) { if (ok()) { f(); chk(hipGetLastError()); } }
    template <class F> void launch_timed(F &&f) {
        if (!ok()) return;
        chk(hipEventRecord(e0, st));
        f();
        chk(hipGetLastError());
        chk(hipEventRecord(e1, st));
    }
    void elapsed(float *ms) { if (ok() && ms) chk(hipEventElapsedTime(ms, e0, e1)); }
    // waits for everything queued so far and reports its error: for a caller that reads elapsed times or enqueues nothing more
    void sync() { synced = chk(st ? hipStreamSynchronize(st) : hipDeviceSynchronize()); }
    // synchronises (unless sync() just has; what that last wait returns is not the call's error), then gives the events, every
    // buffer and an own stream back; the destructor does it on any other way out
    void close() {
        if (!open) return;
        open = false;
        if (!synced) (void)(st ? hipStreamSynchronize(st) : hipDeviceSynchronize());
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        for (DevBuf &b : bufs) b.release();
        if (own && st) return_stream(st);
    }
    // closes and returns the call's code; the text of a HIP error goes to h (a handle-bound call) or to the calling thread
    int finish(mpc_handle *h = nullptr) {
        close();
        return ok() ? (int)MPC_OK : fail(h, MPC_ERR_HIP, std::string(who) + ": " + hipGetErrorString(err));
    }
};

// ---- programs at fixed points (points.hip) that the engine calls ---------------------------------------------------------------------
// mpc_lp_solve_batch with one more output: tight[n_lp x m] = 1 where a row's slack is nonbasic at the vertex found (nullptr: none)
int lp_batch(int32_t device, int64_t n_lp, int32_t m, int32_t n, const double *A, int32_t shared_A, const double *b, int32_t shared_b,
             const double *c, int32_t shared_c, const uint8_t *eq, int32_t *status, double *x, double *obj, int32_t *iters, int32_t *tight);
// the device pointers and sizes of a handle's QP blocks: W [n_c x n_c], UV [n_c x (n_t + 1)], X0H [n_x x (n_t + 1)], Gt [n_c x n_x]
struct QpProgram { int n_c, n_eq, n_t, n_x; const double *W, *UV, *X0H, *Gt; };
// mpc_qp_solve_batch behind its checks, on stream st of the calling thread's device; h only receives the error text
int qp_batch(mpc_handle *h, hipStream_t st, int n_cu, const QpProgram &P, int64_t m, const double *theta, int32_t *status, double *x,
             double *lambda, uint8_t *active, int32_t *iters);

}  // namespace mpc
