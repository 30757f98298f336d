// level_small.hpp -- a level without host round trips (host code only, no kernels): what level_run_impl of mpcombi_hip.hip tries first for
// every level of at most Knobs::smallpath_max candidates (level_run_small), and the same level as a member of the launches that several
// programs share (batch_prepare / batch_finish around batch_level_launch of batch_level.hip).  Included by mpcombi_hip.hip alone, below
// mpc_handle and the engine's helpers it calls (x1_join, level_record_shape, part_spec, dict_*, level_close, level_stats_common, ...): the
// translation unit stays one.
//
// The classic path (level_classic.hpp) reads a list length back after almost every stage (to size the next launch): six synchronisations
// and ~25 dependent launches per level, 0.3-0.45 ms whatever the level computes -- the fixed cost of the first levels of every program, of
// all of config 2 and of the sub-programs of the mixed-integer enumeration.  Here every list length stays in device memory (h->dcnt, words
// named by DcntWord of batch_level.hpp; the kernels read it there: ThetaArgs::n_dev, DictCache::n_*_dev, RegionStream::n_opt_dev,
// k_verdict's n_dev), launches are sized by the one bound the host knows -- the number of candidates of the level --, buffers by the same
// bound, and the host synchronises ONCE, at the end.  Same kernels, same lists (the single-block compaction / partition kernels keep the
// candidate order), same decisions.  The rare stages whose buffers cannot be bounded cheaply -- the LDS-engine region kernel for
// candidates k_region2 gives up on -- are not part of it: if the level turns out to need them, it is repeated on the classic path
// (deterministic, so the repeat computes the same thing).
//
// SmallRun is the level's context: it lives on level_run_small's stack, is built once per level and owns nothing.  Its member functions
// are the level's stages, in the order level_run_small calls them (DESIGN 3.1 has the map); what a stage leaves for a later one is a
// member, and each member says who sets it and who reads it.  The order of the calls on each stream, and of the host's waits between
// them, is the behaviour of the path: a stage function keeps the order its code had inside level_run_small.  What the single level and
// the batch member do alike -- the set-up of the lists and the KKT buffers, the three buffer pieces, the closing -- are the small_*
// functions both call; where the two differ, the difference is an argument at the call.
#pragma once

namespace {   // (internal linkage: the library exports the C ABI and nothing of this; the free functions are `static` as well, because the
              //  include stands inside the engine's extern "C" block, where the unnamed namespace alone does not keep their names local)

// ---- the launch side of the region stage of a small level beside the next level (mpc_handle::RegionDefer) -------------------------------
// the set's buffers <-> the handle's: in at the start of a deferring level (every launch of the level then takes them as it always
// took the handle's), out before its closing synchronisation (the next level works in the handle's own again)
static void defer_swap(mpc_handle *h, mpc_handle::RegionDefer &d) {
    std::swap(h->kkt_code, d.kkt_code); std::swap(h->kkt_L, d.kkt_L); std::swap(h->part_lists, d.part_lists); std::swap(h->headd, d.headd); std::swap(h->headi, d.headi);
    std::swap(h->epool, d.epool); std::swap(h->kept_g, d.kept_g); std::swap(h->done_g, d.done_g); std::swap(h->dcnt, d.dcnt);
}
// Called by a level before its k_children_write: the launch of the level BEFORE reads that level's frontier, which has been this level's
// children buffer since the hand-over.  A stream wait; the launch ended long ago (it was queued a whole level earlier).
static int defer_join(mpc_handle *h, hipStream_t st) {
    for (auto &d : h->rdefer)
        if (d.pending && !d.joined && d.depth != h->sv_cur) { HIP_TRY(h, hipStreamWaitEvent(st, d.ev_done, 0)); d.joined = true; }
    return MPC_OK;
}
// launches that will not be closed (the level is repeated, the solve abandoned or failed): waited for, their records dropped
static void defer_drain(mpc_handle *h) {
    if (!h->defer_pending()) return;
    (void)hipStreamSynchronize(h->stream3);
    for (auto &d : h->rdefer) d.pending = false;
}

static bool small_path_ok(const mpc_handle *h, long long n, int k, int32_t flags, int32_t gen_children) {
    if (h->kn.no_smallpath || !h->fast || h->kn.force_v1 || h->fast_r < 0 || n < 1 || n > h->kn.smallpath_max) return false;
    if (flags & MPC_LEVEL_GRAPH) return false;
    if (h->kn.test_late > 0 || h->kn.debug_cycles) return false;
    // children and their parent slots are sized by the bound n (n_c - k) candidates of k + 1 indices
    const double child_bytes = (double)n * std::max(h->n_c - k, 1) * (k + 2) * 4.0;
    if (gen_children && child_bytes > 512e6) return false;
    const RecordShape sh = record_shape(h, k);
    const double rec_bytes = (double)n * ((double)sh.fd() * 8.0 + (double)sh.fi() * 4.0 + (double)sh.rows_t() * sh.row_len() * 8.0);
    return rec_bytes <= 2e9;
}

// MPC_DEBUG_SMALL=1: at exit, how many no-round-trip levels had doubtful candidates (re-solved in place by the LDS engine) in their two verdict stages
static std::atomic<long long> g_small_levels{0}, g_small_retry_theta{0}, g_small_retry_x{0}, g_small_retry_cands{0}, g_small_repeats{0}, g_small_repeats_doubtful{0};
static void small_debug_note(const int32_t *cnt_host) {
    static const bool on = [] {
        if (knob_process("MPC_DEBUG_SMALL") == 0.0) return false;
        std::atexit([] { std::fprintf(stderr, "[mpc] small levels %lld: with doubtful candidates after the theta stage %lld, after the (x,theta) stage %lld (candidates %lld); repeated on the classic path %lld (because of doubtful candidates %lld)\n",
                                      g_small_levels.load(), g_small_retry_theta.load(), g_small_retry_x.load(), g_small_retry_cands.load(), g_small_repeats.load(), g_small_repeats_doubtful.load()); });
        return true;
    }();
    if (!on) return;
    const int doubtful_t = cnt_host[DC_DOUBTFUL_T] + cnt_host[DC_DOUBTFUL_FUSED];
    g_small_levels++; g_small_retry_theta += doubtful_t > 0; g_small_retry_x += cnt_host[DC_DOUBTFUL_X] > 0; g_small_retry_cands += doubtful_t + cnt_host[DC_DOUBTFUL_X];
}

// what the two forms without host round trips add alike to level_stats_common: the work-item counts from the published list lengths,
// k_region2's own wall-clock time, the dictionary traffic
static void level_stats_small(const mpc_handle *h, const LevelCounters &host_ctr, const int32_t *cnt_host, bool kkt, bool quick_test, mpc_level_stats *stats) {
    level_stats_common(h, host_ctr, stats);
    stats->n_xtheta_lp = h->n_needx;
    stats->n_theta_items = kkt ? cnt_host[DC_THETA] : h->n;
    if (h->n_opt > 0 && host_ctr.r2_t1 > ~host_ctr.r2_not_t0 && h->wall_khz > 0)   // k_region2 times itself on the wall clock
        stats->ms_region2 = (float)((double)(host_ctr.r2_t1 - ~host_ctr.r2_not_t0) / (double)h->wall_khz);
    stats->n_xq_items = quick_test ? cnt_host[DC_OPEN] : 0;
    stats->n_x_items = (quick_test ? cnt_host[DC_OPEN_QT] : cnt_host[DC_OPEN]) + (h->storing ? (long long)cnt_host[DC_FEASIBLE] + cnt_host[DC_OPT] : 0);
    stats->dict_read_bytes = (h->have_prev_dict && h->have_parent_slot) ? dict_record_bytes(h) : 0;
    stats->dict_write_bytes = h->storing ? dict_record_bytes(h) : 0;
}

// ==== the set-up and the closing that level_run_small and batch_prepare / batch_finish share ================================================
// The buffer set-up comes in pieces, not as one function: level_run_small queues launches between them, and each piece stands where its
// lines stood, so that no ensure call has moved past a launch on the member's stream.
static void small_reset_counts(mpc_handle *h) {
    h->n_opt = h->n_children = h->n_pruned_new = h->n_regions = 0;
    h->n_needx = 0;
}
// status, pruned masks and the work lists by the bound nn; the list lengths (dcnt_bytes: DCNT_BYTES, or with a deferred launch's counters behind them)
static int small_level_lists(mpc_handle *h, size_t nn, hipStream_t st, size_t dcnt_bytes) {
    HIP_TRY(h, h->status.ensure(nn, st));
    HIP_TRY(h, h->pruned.ensure((size_t)(h->n_pruned + nn) * h->mw * sizeof(uint64_t), st, true));   // the level's newly pruned masks go behind the list
    HIP_TRY(h, h->retry_list.ensure(nn * sizeof(int32_t), st));
    HIP_TRY(h, h->theta_list.ensure(nn * sizeof(int32_t), st));
    HIP_TRY(h, h->part_lists.ensure((size_t)PART_CLASSES * nn * sizeof(int32_t), st));
    HIP_TRY(h, h->dcnt.ensure(dcnt_bytes, st));
    return MPC_OK;
}
// does the level solve its KKT systems with one thread per candidate (k_kkt_thread)?  kd: the rows it solves for (the equality rows are
// eliminated); max_rows, off: the caller's limit and its reading of MPC_NO_KKT_THREAD
static bool small_kkt_on(const mpc_handle *h, int kd, int max_rows, bool off) { return h->kkt_mode == 0 && kd >= 1 && kd <= max_rows && !off; }
// k_kkt_thread's codes and multipliers; `listed`: the kernel lists the candidates it leaves to the theta stage itself, into ta (one atomic
// per workgroup; a work list: its order changes nothing)
static int small_kkt_buffers(mpc_handle *h, size_t nn, int k, hipStream_t st, int32_t *dcnt, ThetaArgs &ta, bool &listed) {
    HIP_TRY(h, h->kkt_code.ensure(nn, st));
    HIP_TRY(h, h->kkt_L.ensure(nn * (size_t)k * (h->n_t + 1) * sizeof(double), st));
    listed = !h->kn.no_kkt_lists;
    if (listed) {
        HIP_TRY(h, h->xq_list.ensure(nn * sizeof(int32_t), st));
        ta.kt_list = h->theta_list.as<int32_t>(); ta.kt_n = dcnt + DC_THETA;
        ta.kx_list = h->xq_list.as<int32_t>(); ta.kx_n = dcnt + DC_KX;
    }
    return MPC_OK;
}
// region stage: one slot per optimal candidate (class 2 of the partition behind the theta stage), buffers sized by the bound nn
static int small_region_slots(mpc_handle *h, size_t nn, hipStream_t st, int &ldk) {
    h->opt_ptr = h->part_lists.as<int32_t>() + 2 * nn;
    const int rows_t_ = h->n_c - h->n_eq + h->n_tc;
    HIP_TRY(h, h->headd.ensure(nn * h->fd * sizeof(double), st));
    HIP_TRY(h, h->headi.ensure(nn * h->fi * sizeof(int32_t), st));
    HIP_TRY(h, h->epool.ensure(nn * rows_t_ * (h->n_t + 1) * sizeof(double), st));
    ldk = (rows_t_ + 1 + 63) & ~63;
    HIP_TRY(h, h->kept_g.ensure(nn * ldk, st));
    HIP_TRY(h, h->done_g.ensure(nn * 2 * sizeof(unsigned int), st));
    h->used_region2 = true;
    return MPC_OK;
}
// (x,theta) stage: the dictionary cache; on a storing level the candidates the theta stage decided (classes 1 and 2) ride in front of the open ones
static int small_dict_cache(mpc_handle *h, size_t nn, int32_t gen_children, hipStream_t st, int32_t *dcnt, DictCache &dc) {
    { int rcd = dict_cache_begin(h, nn, gen_children, st, dc); if (rcd) return rcd; }
    if (h->storing) {
        dc.pre1 = h->part_lists.as<int32_t>() + 1 * nn; dc.n_pre1_dev = dcnt + DC_FEASIBLE;
        dc.pre2 = h->part_lists.as<int32_t>() + 2 * nn; dc.n_pre2_dev = dcnt + DC_OPT;
    }
    dc.chunk = 1;
    return MPC_OK;
}
// children stage: masks, counts, offsets, and children with their parent slots by the bound nn (n_c - k)
static int small_children_buffers(mpc_handle *h, size_t nn, int k, hipStream_t st) {
    HIP_TRY(h, h->childmask.ensure(nn * h->mw * sizeof(uint64_t), st));
    HIP_TRY(h, h->count.ensure(nn * sizeof(int32_t), st));
    HIP_TRY(h, h->offset.ensure(nn * sizeof(int32_t), st));
    const size_t child_bound = nn * (size_t)std::max(h->n_c - k, 1);
    HIP_TRY(h, h->children.ensure(child_bound * (k + 1) * sizeof(int32_t), st));
    HIP_TRY(h, h->parent_slot_next.ensure(child_bound * sizeof(int32_t), st));
    return MPC_OK;
}
// behind the level's one synchronisation: the counters as its closing publish left them in the pinned block; returns the list lengths beside them
static const int32_t *small_read_counters(mpc_handle *h, LevelCounters &host_ctr) {
    std::memcpy(&host_ctr, h->tot_host + 16, sizeof(LevelCounters));
    const int32_t *cnt_host = h->cnt_host();
    h->n_smallpath++;
    small_debug_note(cnt_host);
    return cnt_host;
}
// what a level that ran to its end leaves on the handle; word_opt: where the form counts its optimal candidates
static void small_take_counts(mpc_handle *h, int32_t gen_children, const LevelCounters &host_ctr, const int32_t *cnt_host, DcntWord word_opt) {
    h->n_opt = cnt_host[word_opt];
    h->n_children = gen_children ? cnt_host[DC_CHILDREN] : 0;
    h->n_needx = cnt_host[DC_OPEN];
    h->n_pruned_new = host_ctr.n_pruned_new;
    h->n_erows = host_ctr.e_rows;
    h->n_regions = (long long)host_ctr.status[ST_REGION];
}

// ==== one level of one program ================================================================================================================
struct SmallRun {
    // ---- per-level constants (set by the constructor) ---------------------------------------------------------------------------------------
    mpc_handle *const h;            // the handle
    const int32_t gen_children;     // the level generates children (the next level's candidates)
    const int32_t flags;            // MPC_LEVEL_* of the call
    const long long n;              // candidates of the level
    const int k;                    // their cardinality
    const size_t nn;                // n as a size
    const hipStream_t st;           // the handle's main stream
    // Round 5 (`fused`): doubtful candidates are rare (numerically doubtful pivots of the register simplex), so the level does not spend
    // three launches on them at each of its two verdict stages (resolve_doubtful): ONE partition lists them as class 0 beside the others,
    // the level goes on without them, and if there was one (DC_DOUBTFUL_FUSED / DC_DOUBTFUL_X) the host repeats the level on the classic
    // path -- as it does for the other rare cases.  The end of the level is one launch (k_small_end) instead of five, the scan carries the
    // publish.  Not fused: the round-4 form, on a handle with an open parameter set or one that has met a doubtful candidate.
    const bool fused;
    const bool will_store;          // the level keeps its dictionaries for its children (small_dict_cache decides the same: h->storing)
    const int keep_lowdim;          // MPC_LEVEL_KEEP_LOWDIM of the call, as the kernels take it
    const int blocks256;            // blocks of 256 candidates
    unsigned int *const pub_dst;    // where the closing publish writes: the counters' place in the pinned block (device alias)
    // ---- stage to stage -----------------------------------------------------------------------------------------------------------------------
    mpc_handle::RegionDefer *df = nullptr;   // set by begin: the set the level's region launch is deferred in (nullptr: in line); read by begin, first_partition, region_args, region_launch, children, publish_and_wait, verdict, take_counts, fill_stats
    LevelCounters *ctr = nullptr;   // set by begin: the level's counters on the device; read by every stage
    int32_t *dcnt = nullptr;        // set by begin: the device-resident list lengths (DcntWord; the deferring set's while df); read by every stage
    const int32_t *fr = nullptr;    // set by begin: the frontier; read by every stage
    uint8_t *stp = nullptr;         // set by begin: the status array; read by every stage
    const DevProblem *pf = nullptr; // set by begin: k_verdict2's view of the program on the device; read by kkt_stage, theta_stage, region_launch, quick_test_stage, x_stage
    const uint8_t *kkc = nullptr;   // set by kkt_stage: KKT codes and multipliers of k_kkt_thread (nullptr: the theta kernel solves); read by theta_stage, region_args, fill_stats
    const double *kkl = nullptr;    // set by kkt_stage, with kkc
    ThetaArgs ta{};                 // set by kkt_stage: k_theta2's arguments (the list's length on the device if k_kkt_thread ran); read by theta_stage
    const int32_t *theta_list = nullptr;   // set by kkt_stage: the theta stage's work list (nullptr: every candidate); read by theta_stage
    SmallRX rx{};                   // set by region_args (k_region2's arguments), region_launch (k_x2's, for the merged grid); read by region_launch, region2_alone
    unsigned grid_r = 1;            // set by region_args: workgroups of the region launch; read by region_launch, region2_alone
    LevelCounters *ctr_r = nullptr; // set by region_args: where the region launch counts (a deferred one: behind the set's list lengths); read by region_launch
    DictCache dc{};                 // set by x_cache: the dictionary cache of the (x,theta) stage; read by region_launch, quick_test_stage, x_stage
    const int32_t *needx_list = nullptr;   // set by x_cache, quick_test_stage: the candidates whose feasibility is open; read by region_launch, quick_test_stage, x_stage
    const int32_t *needx_n = nullptr;      // set by x_cache, quick_test_stage: their number, on the device; read by region_launch, quick_test_stage, x_stage
    bool quick_test = false;        // set by x_cache: the level ends with the quick test (last level: decisions only); read by region_launch, quick_test_stage, fill_stats
    bool merged_rx = false;         // set by region_launch: k_region2 and k_x2 went out as one grid; read by x_stage
    const int32_t *cnt_host = nullptr;     // set by verdict: the list lengths as published; read by take_counts, fill_stats
    LevelCounters host_ctr;         // set by verdict: the counters as published; read by take_counts, fill_stats
    float ms[3] = {0, 0, 0};        // set by take_counts: verdict / region / children times between ev[0..3]; read by fill_stats

    SmallRun(mpc_handle *h_, int32_t gen_children_, int32_t flags_)
        : h(h_), gen_children(gen_children_), flags(flags_), n(h_->n), k(h_->k), nn((size_t)h_->n), st(h_->stream),
          fused(!h_->theta_open && !h_->kn.no_small_fuse), will_store(dict_will_store(h_, (size_t)h_->n, gen_children_)),
          keep_lowdim((flags_ & MPC_LEVEL_KEEP_LOWDIM) ? 1 : 0), blocks256((int)((h_->n + 255) / 256)),
          pub_dst(reinterpret_cast<unsigned int *>(h_->tot_dev + 16)) {
        std::memset(&host_ctr, 0, sizeof(host_ctr));
    }

    // ==== helpers ==============================================================================================================================
    int32_t *part_list(int c) const { return h->part_lists.as<int32_t>() + (size_t)c * nn; }
    bool doubtful_seen() const { return fused && (cnt_host[DC_DOUBTFUL_FUSED] > 0 || cnt_host[DC_DOUBTFUL_X] > 0); }

    int region2_alone(hipStream_t rst) {
        launch_region2(h->fast_r, dim3(grid_r), h->lds_r2, rst, rx.pr, rx.fr, rx.k, rx.opt_list, rx.n, rx.status, rx.headd, rx.headi, rx.fd, rx.fi, rx.epool,
                       rx.ctr, rx.kkc, rx.kkl, rx.W, rx.kept_g, rx.ldk, rx.done_g, rx.tvp_box, rx.rs);
        HIP_TRY(h, hipGetLastError());
        return MPC_OK;
    }

    // Round-4 form only: the doubtful candidates of a verdict stage (rare) are re-solved in place by the LDS engine (the classic path does
    // this on a side stream under the (x,theta) stage), so that the partition that follows already knows every optimal candidate they
    // yield.  cnt: their number, class 0 of a partition of its own.  then_recession (behind the theta stage only): on an open parameter
    // set "optimal" holds only if the reference's max-t LP is bounded (k_recession), decided before the region launch.
    int resolve_doubtful(int32_t *cnt, bool then_recession) {
        if (fused) return MPC_OK;
        hipLaunchKernelGGL(k_partition_small, dim3(1), dim3(1024), 0, st, h->status.as<uint8_t>(), (int)n, part_spec({{ST_RETRY, 0}}), h->part_lists.as<int32_t>(), (long long)n, cnt);
        hipLaunchKernelGGL(k_verdict, dim3((unsigned)std::min<long long>(n, 128)), dim3(64), h->lds_v, st, h->Pv, fr, n, k, stp, ctr, part_list(0), cnt);
        if (then_recession && h->theta_open) hipLaunchKernelGGL(k_recession, dim3((unsigned)std::min<long long>(n, 256)), dim3(64), h->lds_v, st, h->Pv, fr, n, k, stp);
        return MPC_OK;
    }

    // ==== stages, in the order of the level ====================================================================================================
    // the deferred k_x1 joined, the deferral decided (its set's buffers swapped in), buffers by the bound, everything cleared by one launch
    int begin() {
        { int rcj = x1_join(h); if (rcj) return rcj; }
        small_reset_counts(h);
        // The region stage beside the NEXT level (mpc_handle::RegionDefer): inside mpc_solve_start's loop, on a level with children in the fused
        // form that does not end with the quick test; not under a profile (per-stage events in line, as for the deferred k_x1), not where the next
        // level's launches depend on this level's number of regions (MPC_XQ_EARLY_REGIONS).
        if (h->sv_cur >= 0 && h->defer_mode > 0 && !h->defer_off && !h->kn.no_roverlap && gen_children && fused && !h->timing && h->kn.xq_early_regions == 0 &&
            (will_store || !(h->have_prev_dict && h->have_parent_slot))) {
            df = &h->rdefer[h->sv_cur & 1];
            if (df->pending) return fail(h, MPC_ERR_STATE, "level_run_small: the deferred region launch of two levels ago has not been closed");
            defer_swap(h, *df);
        }
        { int rcb = small_level_lists(h, nn, st, mpc_handle::DEFER_DCNT_BYTES); if (rcb) return rcb; }
        {
            // counters, list lengths, the region kernel's completion flags and the "dictionary stored" flags: cleared by one launch
            HIP_TRY(h, h->done_g.ensure(nn * 2 * sizeof(unsigned int), st));
            if (will_store) HIP_TRY(h, h->dict_stored[h->dict_cur].ensure(nn, st));
            ZeroBufs z{};
            z.p[0] = h->ctr.p; z.bytes[0] = sizeof(LevelCounters);
            z.p[1] = h->dcnt.p; z.bytes[1] = df ? mpc_handle::DEFER_DCNT_BYTES : DCNT_BYTES;   // (a deferred launch counts in its own LevelCounters, behind the list lengths)
            z.p[2] = h->done_g.p; z.bytes[2] = nn * 2 * sizeof(unsigned int);
            if (will_store) { z.p[3] = h->dict_stored[h->dict_cur].p; z.bytes[3] = nn; }
            hipLaunchKernelGGL(k_zero_bufs, dim3((unsigned)std::min<size_t>(64, (nn * 8 + 2047) / 2048 + 1)), dim3(256), 0, st, z);
        }
        ctr = h->ctr.as<LevelCounters>();
        dcnt = h->dcnt.as<int32_t>();
        fr = h->frontier.as<int32_t>();
        stp = h->status.as<uint8_t>();
        pf = h->pf_dev.as<DevProblem>();
        level_record_shape(h, k);
        if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[0], st));
        return MPC_OK;
    }

    // KKT solves + box screen, one thread (or KKT_SPREAD lanes) per candidate; the theta kernel fetches the multipliers of what the screen left open
    int kkt_stage() {
        ta = h->targs;
        ta.chunk = 1;
        const int kd = k - h->targs.ne;   // rows the one-thread KKT kernel solves for (the equality rows are eliminated)
        if (!small_kkt_on(h, kd, KKT_THREAD_MAX, h->kn.no_kkt_thread != 0)) return MPC_OK;
        ThetaArgs tk = h->targs;
        bool kkt_lists = false;
        { int rcb = small_kkt_buffers(h, nn, k, st, dcnt, tk, kkt_lists); if (rcb) return rcb; }
        kkc = h->kkt_code.as<uint8_t>(); kkl = h->kkt_L.as<double>();
        // KKT_SPREAD lanes per candidate while the active set is small (the kernel's comment): the level's 50 us floor becomes ~15
        const bool spread = h->kn.kkt_spread > 0 && kd <= KKT_SPREAD_KMAX;
        const dim3 g((unsigned)(spread ? (n * KKT_SPREAD + 255) / 256 : blocks256));
        launch_kkt_thread(kd, h->fast_t, spread, g, st, pf, fr, n, h->kkt_code.as<uint8_t>(), h->kkt_L.as<double>(), stp, tk, ctr);
        if (!kkt_lists) hipLaunchKernelGGL(k_compact_small, dim3(1), dim3(1024), 0, st, h->status.as<uint8_t>(), (int)n, ST_TODO, ST_TODO, h->theta_list.as<int32_t>(), dcnt + DC_THETA);
        theta_list = h->theta_list.as<int32_t>();
        ta.n_dev = dcnt + DC_THETA;
        return MPC_OK;
    }

    int theta_stage() {
        launch_theta2(h->fast_t, dim3((unsigned)std::min<long long>(n, h->grid_f)), h->lds_f, st, pf, fr, n, k, stp, ctr, kkc, kkl, ta, theta_list);
        return MPC_OK;
    }

    // classes after the theta stage: [1] feasible, [2] optimal, [3] feasibility open ([0] doubtful, fused form only)
    int first_partition() {
        hipLaunchKernelGGL(k_partition_small, dim3(1), dim3(1024), 0, st, h->status.as<uint8_t>(), (int)n,
                           fused ? part_spec({{ST_RETRY, 0}, {ST_FEASIBLE, 1}, {ST_OPT_PENDING, 2}, {ST_NEEDX, 3}, {ST_NEEDX_SING, 3}})
                                 : part_spec({{ST_FEASIBLE, 1}, {ST_OPT_PENDING, 2}, {ST_NEEDX, 3}, {ST_NEEDX_SING, 3}}), h->part_lists.as<int32_t>(), (long long)n, dcnt + DC_CLASS);
        HIP_TRY(h, hipGetLastError());
        if (df) HIP_TRY(h, hipEventRecord(df->ev_go, st));   // everything the deferred region launch reads has been queued
        return MPC_OK;
    }

    // Region stage: one slot per optimal candidate, buffers sized by the bound.  It needs the theta stage's verdicts only; a candidate that
    // turns out optimal only later -- a doubtful one of the (x,theta) stage, re-solved -- sends the level to the classic path.  (Measured:
    // on its own stream beside the (x,theta) stage it gains nothing at this size -- the fork / join events cost what the overlap of two
    // 50-100 us kernels saves: config 2 1.76 ms against 1.68 in line; round 4, config 4, whose regions take 150 us: 5.47 / 5.61 ms forked
    // against 5.48 / 5.54 in line -- the region kernel itself is 0.185 instead of 0.158 ms beside k_x2.)  The launch itself is region_launch's.
    int region_args() {
        // a deferred launch counts in its own LevelCounters (the next level clears the handle's) and leaves status[] alone (the next level's by then)
        ctr_r = df ? reinterpret_cast<LevelCounters *>(h->dcnt.as<char>() + DCNT_BYTES) : ctr;
        int ldk = 0;
        { int rcb = small_region_slots(h, nn, st, ldk); if (rcb) return rcb; }
        RegionStream rs{};
        rs.n_opt_dev = dcnt + DC_OPT;
        rs.w_cap = h->grid_r2; rs.w_max = h->kn.rsplit_max;
        const int W = h->kn.no_rsplit ? 1 : 0;   // 0: chosen in the kernel from the number of optimal candidates
        grid_r = (unsigned)std::min<long long>(n * std::max(h->kn.rsplit_max, 1), h->grid_r2);
        const DevProblem *pr = h->pr2_dev.as<DevProblem>();
        const int nt_r = region2_nt(h->fast_r);
        rx.pr = pr; rx.fr = h->frontier.as<int32_t>(); rx.k = k; rx.opt_list = h->opt_ptr; rx.n = (int)n; rx.status = df ? (uint8_t *)nullptr : h->status.as<uint8_t>();
        rx.headd = h->headd.as<double>(); rx.headi = h->headi.as<int32_t>(); rx.fd = h->fd; rx.fi = h->fi; rx.epool = h->epool.as<double>(); rx.ctr = ctr_r;
        rx.kkc = kkc; rx.kkl = kkl; rx.W = W; rx.kept_g = h->kept_g.as<uint8_t>(); rx.ldk = ldk; rx.done_g = h->done_g.as<unsigned int>();
        rx.tvp_box = h->kn.no_rbox ? (const double *)nullptr : h->targs.tvp + (size_t)nt_r * nt_r + nt_r; rx.rs = rs;
        return MPC_OK;
    }

    // the dictionary cache of the (x,theta) stage, the list of the open candidates, and whether the level ends with the quick test
    int x_cache() {
        if (!fused) HIP_TRY(h, hipMemsetAsync(&ctr->work_retry, 0, sizeof(unsigned int), st));   // (k_verdict's work counter, between its two launches)
        { int rcb = small_dict_cache(h, nn, gen_children, st, dcnt, dc); if (rcb) return rcb; }
        needx_list = part_list(3);
        needx_n = dcnt + DC_OPEN;
        quick_test = !h->storing && dc.parent_slot;
        return MPC_OK;
    }

    // k_region2 in one of three placements: deferred on stream3, merged with k_x2 in one grid where an instantiation of the pair exists, or alone
    int region_launch() {
        if (df) return region_deferred();
        if (fused && !quick_test && !h->kn.no_small_rx) {
            // region kernel + (x,theta) kernel as ONE grid (batch_level.hpp, SmallRX): the two work on disjoint candidates
            DictCache d = dc;
            d.n_list_dev = needx_n;
            rx.pf = pf; rx.list = needx_list; rx.dc = d;
            hipError_t e_rx = hipSuccess;
            merged_rx = small_region2_x2_launch(h->fast_r, h->fast_x, grid_r, (unsigned)std::min<long long>(n, (long long)h->n_cu * 16), h->lds_r2, st, rx, &e_rx);
            if (merged_rx) { HIP_TRY(h, e_rx); return MPC_OK; }
        }
        return region2_alone(st);
    }
    // stream3, behind the partition's event: the main stream goes on with k_x2 and the end of the level and never waits for this
    // launch inside the level.  Behind it, on the same stream, what the host needs to close the level goes to the pinned block.
    int region_deferred() {
        HIP_TRY(h, hipStreamWaitEvent(h->stream3, df->ev_go, 0));
        { int rcr = region2_alone(h->stream3); if (rcr) return rcr; }
        hipLaunchKernelGGL(k_defer_publish, dim3(1), dim3(256), 0, h->stream3, rx.headi, rx.fi, rx.rs.n_opt_dev, reinterpret_cast<const unsigned int *>(ctr_r),
                           (int)(sizeof(LevelCounters) / 4), h->defer_pub_dev(h->sv_cur & 1));
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipEventRecord(df->ev_done, h->stream3));
        df->pending = true; df->joined = false; df->depth = h->sv_cur; df->k = k; df->fd = h->fd; df->fi = h->fi; df->n_opt = 0;
        df->keep_lowdim = keep_lowdim;
        return MPC_OK;
    }

    // last level: decisions only -- the quick test on a few vectors of the parent's dictionary first (k_xq), what it leaves open listed again
    int quick_test_stage() {
        if (!quick_test) return MPC_OK;
        DictCache dq = dc;
        dq.n_list_dev = needx_n;
        const dim3 gg((unsigned)std::min<long long>(n, (long long)h->n_cu * 32));
        launch_xq(h->fast_x, gg, st, pf, fr, k, needx_list, (int)n, stp, ctr, dq, dict_nxc(h));
        hipLaunchKernelGGL(k_compact_small, dim3(1), dim3(1024), 0, st, h->status.as<uint8_t>(), (int)n, ST_NEEDX, ST_NEEDX_SING, h->retry_list.as<int32_t>(), dcnt + DC_OPEN_QT);
        needx_list = h->retry_list.as<int32_t>();
        needx_n = dcnt + DC_OPEN_QT;
        return MPC_OK;
    }

    // k_x2, unless it went out with the region kernel
    int x_stage() {
        if (!merged_rx) {
            DictCache d = dc;
            d.n_list_dev = needx_n;
            // bound of the work items: every candidate once (open, or decided and expanded for its dictionary)
            launch_x2(h->fast_x, dim3((unsigned)std::min<long long>(n, (long long)h->n_cu * 16)), st, pf, fr, k, needx_list, (int)n, stp, ctr, d);
        }
        HIP_TRY(h, hipGetLastError());
        return MPC_OK;
    }

    int end_of_level() { return fused ? end_fused() : end_round4(); }
    // doubtful candidates of the (x,theta) stage -> DC_DOUBTFUL_X, optimal ones that missed the region launch -> DC_LATE, status histogram,
    // pruned masks (and, on a level without children, the publish): one launch
    int end_fused() {
        if (h->timing) { HIP_TRY(h, hipEventRecord(h->ev[1], st)); HIP_TRY(h, hipEventRecord(h->ev[2], st)); }
        unsigned long long *pout = h->pruned.as<unsigned long long>() + (size_t)h->n_pruned * h->mw;
        launch_small_end(h->mw, st, fr, (int)n, k, stp, pout, ctr, keep_lowdim, dcnt + DC_DOUBTFUL_X, dcnt + DC_LATE, reinterpret_cast<const unsigned int *>(dcnt), DCNT_WORDS,
                         gen_children ? (unsigned int *)nullptr : pub_dst);
        HIP_TRY(h, hipGetLastError());
        return MPC_OK;
    }
    // behind resolve_doubtful: the late optimal candidates counted, the pruned masks of this level
    int end_round4() {
        HIP_TRY(h, hipGetLastError());
        if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[1], st));
        // a candidate that is still "optimal, region pending" now was not in the region launch: counted in DC_LATE
        hipLaunchKernelGGL(k_partition_small, dim3(1), dim3(1024), 0, st, h->status.as<uint8_t>(), (int)n, part_spec({{ST_OPT_PENDING, 1}}), h->part_lists.as<int32_t>(), (long long)n, dcnt + DC_LATE_CLASS);
        HIP_TRY(h, hipGetLastError());
        if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[2], st));
        launch_pruned_append(h->mw, dim3(blocks256), st, h->frontier.as<int32_t>(), n, k, h->status.as<uint8_t>(),
                             h->pruned.as<unsigned long long>() + (size_t)h->n_pruned * h->mw, ctr, keep_lowdim);
        return MPC_OK;
    }

    // count, scan (in the fused form it carries the level's publish), write
    int children() {
        if (!gen_children) return MPC_OK;
        { int rcb = small_children_buffers(h, nn, k, st); if (rcb) return rcb; }
        // (deferred region launch: the optimal candidates are still "region pending" here and expand as if they had their regions)
        launch_children_count(h->mw, dim3((unsigned)n), st, h->Pv, h->frontier.as<int32_t>(), n, k, h->status.as<uint8_t>(),
                              h->pruned.as<unsigned long long>(), (long long)h->n_pruned, h->childmask.as<unsigned long long>(), h->count.as<int32_t>(),
                              keep_lowdim | (df ? EXPAND_PENDING : 0));
        if (fused) hipLaunchKernelGGL(k_scan_publish, dim3(1), dim3(SCAN_BLOCK), 0, st, h->count.as<int32_t>(), h->offset.as<int32_t>(), (int)n, dcnt + DC_CHILDREN,
                                      reinterpret_cast<const unsigned int *>(ctr), (int)(sizeof(LevelCounters) / 4), reinterpret_cast<const unsigned int *>(dcnt), DCNT_WORDS, pub_dst);
        else hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(SCAN_BLOCK), 0, st, h->count.as<int32_t>(), h->offset.as<int32_t>(), (int)n, dcnt + DC_CHILDREN);
        { int rcj = defer_join(h, st); if (rcj) return rcj; }   // the children buffer is the frontier the previous level's deferred region launch reads
        hipLaunchKernelGGL(k_children_write, dim3((unsigned)n), dim3(64), 0, st, h->frontier.as<int32_t>(), n, k, h->mw,
                           h->childmask.as<unsigned long long>(), h->offset.as<int32_t>(), h->children.as<int32_t>(),
                           h->storing ? h->dict_stored[h->dict_cur].as<uint8_t>() : (const uint8_t *)nullptr, h->parent_slot_next.as<int32_t>());
        HIP_TRY(h, hipGetLastError());
        return MPC_OK;
    }

    // round 4: the status histogram, and counters and list lengths to the pinned block (the fused form has published: k_small_end or the scan)
    int publish_round4() {
        hipLaunchKernelGGL(k_histogram, dim3(std::min(blocks256, 1024)), dim3(256), 0, st, h->status.as<uint8_t>(), n, ctr);
        if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[3], st));
        hipLaunchKernelGGL(k_publish_words2, dim3(1), dim3(128), 0, st, reinterpret_cast<const unsigned int *>(ctr), (int)(sizeof(LevelCounters) / 4),
                           reinterpret_cast<const unsigned int *>(dcnt), DCNT_WORDS, pub_dst);
        return MPC_OK;
    }
    int publish_and_wait() {
        if (!fused) { int rcp = publish_round4(); if (rcp) return rcp; }
        else if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[3], st));
        HIP_TRY(h, hipGetLastError());
        if (df) defer_swap(h, *df);   // every launch is queued: the set keeps what its region launch works in, the handle has its own buffers back
        HIP_TRY(h, hipStreamSynchronize(st));   // the level's only synchronisation
        return MPC_OK;
    }

    // the counters as published; *fallback: the level is repeated on the classic path
    int verdict(bool *fallback) {
        cnt_host = small_read_counters(h, host_ctr);
        if (doubtful_seen()) { h->n_smallpath_doubtful++; g_small_repeats_doubtful++; }
        // (behind a deferred region launch every optimal candidate is still "region pending": exactly the launch's, DC_OPT, may be)
        const int n_late = cnt_host[DC_LATE] - (df ? cnt_host[DC_OPT] : 0);
        if (!(host_ctr.n_rretry > 0 || n_late != 0 || h->kn.test_small_fallback || doubtful_seen())) return MPC_OK;
        // a candidate k_region2 gave up on (the LDS-engine region kernel is not part of this path), or one that turned out optimal
        // after the region launch: the level is repeated classically
        if (df) { HIP_TRY(h, hipEventSynchronize(df->ev_done)); df->pending = false; }   // its own deferred launch: waited for, its records dropped
        h->n_smallpath_fallback++; g_small_repeats++;
        // The repeat must not look for other parents' records: this run's k_children_write has overwritten the previous level's frontier
        // (it lives in the children buffer since the hand-over), which that search walks.
        h->n_prev = 0;
        // A program that produces doubtful candidates keeps doing so (measured: 10-17 % of the small levels of random mpQPs, none on the
        // named configurations): its handle goes back to re-solving them in place, so the repeat is paid once per handle.
        if (doubtful_seen()) h->kn.no_small_fuse = true;
        *fallback = true;
        return MPC_OK;
    }

    // the stage times, what the level leaves on the handle, the end of the level
    int take_counts() {
        if (h->timing) HIP_TRY(h, hipEventElapsedTime(&ms[0], h->ev[0], h->ev[1]));
        if (h->timing) HIP_TRY(h, hipEventElapsedTime(&ms[1], h->ev[1], h->ev[2]));
        if (h->timing) HIP_TRY(h, hipEventElapsedTime(&ms[2], h->ev[2], h->ev[3]));
        small_take_counts(h, gen_children, host_ctr, cnt_host, DC_OPT);
        if (df) df->n_opt = h->n_opt;   // (regions, rows, the launch's counters: defer_close, behind the next level)
        level_close(h, n);
        return MPC_OK;
    }

    void fill_stats(mpc_level_stats *stats) const {
        level_stats_small(h, host_ctr, cnt_host, kkc != nullptr, quick_test, stats);
        stats->ms_verdict = ms[0]; stats->ms_region = ms[1]; stats->ms_children = ms[2]; stats->ms_total = ms[0] + ms[1] + ms[2];
        if (df) stats->region_side_stream = 2;
    }
};

static int level_run_small(mpc_handle *h, int32_t gen_children, int32_t flags, mpc_level_stats *stats, bool *fallback) {
    *fallback = false;
    SmallRun lv(h, gen_children, flags);
    if (int rc = lv.begin()) return rc;                                            // x1_join, the deferral's gate, buffers, k_zero_bufs
    if (int rc = lv.kkt_stage()) return rc;                                        // k_kkt_thread (k_compact_small)
    if (int rc = lv.theta_stage()) return rc;                                      // k_theta2
    if (int rc = lv.resolve_doubtful(lv.dcnt + DC_DOUBTFUL_T, true)) return rc;    // round 4: k_partition_small, k_verdict, k_recession
    if (int rc = lv.first_partition()) return rc;                                  // k_partition_small; the deferred launch's go
    if (int rc = lv.region_args()) return rc;                                      // region slots, k_region2's arguments
    if (int rc = lv.x_cache()) return rc;                                          // dictionary cache, the open list
    if (int rc = lv.region_launch()) return rc;                                    // k_region2: on stream3 with k_defer_publish / with k_x2 in one grid / alone
    if (int rc = lv.quick_test_stage()) return rc;                                 // last level: k_xq, k_compact_small
    if (int rc = lv.x_stage()) return rc;                                          // k_x2
    if (int rc = lv.resolve_doubtful(lv.dcnt + DC_DOUBTFUL_X, false)) return rc;   // round 4: k_partition_small, k_verdict
    if (int rc = lv.end_of_level()) return rc;                                     // k_small_end / round 4: k_partition_small, k_pruned_append
    if (int rc = lv.children()) return rc;                                         // k_children_count, k_scan_publish / k_scan_small, k_children_write
    if (int rc = lv.publish_and_wait()) return rc;                                 // round 4: k_histogram, k_publish_words2; the level's one synchronisation
    if (int rc = lv.verdict(fallback)) return rc;                                  // the counters as published; repeat on the classic path?
    if (*fallback) return MPC_OK;
    if (int rc = lv.take_counts()) return rc;                                      // what the level leaves on the handle; level_close
    if (stats) lv.fill_stats(stats);
    return MPC_OK;
}

// ---- the same level for many programs at once (batch_level.hpp) -----------------------------------------------------------------
// batch_prepare = level_run_small up to its first launch (buffers and arguments: the small_* pieces above, in SmallRun's order),
// batch_finish = level_run_small after its one synchronisation; the launches in between are batch_level_launch's, one per stage for all
// members.  A member has no deferral and no x1_join (a batch runs no classic level that could leave a k_x1 behind), clears DCNT_BYTES of
// list lengths, solves at most BATCH_KKT_THREAD_MAX rows per thread, builds ALL its optimal candidates last (DC_BATCH_OPT) and keeps retry
// slots for what k_region2 gives up on (DC_BATCH_RRETRY).
static int batch_prepare(mpc_handle *h, int32_t gen_children, int32_t flags, BatchMember &m) {
    const long long n = h->n;
    const int k = h->k;
    const size_t nn = (size_t)n;
    hipStream_t st = h->stream;
    std::memset(&m, 0, sizeof(m));
    small_reset_counts(h);
    { int rcb = small_level_lists(h, nn, st, DCNT_BYTES); if (rcb) return rcb; }
    level_record_shape(h, k);
    m.k = k; m.kd = k - h->targs.ne; m.fast_t = h->fast_t; m.fast_x = h->fast_x; m.fast_r = h->fast_r; m.mw = h->mw;
    m.gen_children = gen_children ? 1 : 0;
    m.n = n; m.grid_f = h->grid_f; m.grid_r2 = h->grid_r2; m.n_cu = h->n_cu; m.lds_f = h->lds_f; m.lds_v = h->lds_v; m.lds_r2 = h->lds_r2;
    m.rsplit_max = h->kn.rsplit_max;
    m.pf = h->pf_dev.as<DevProblem>(); m.pr = h->pr2_dev.as<DevProblem>(); m.Pv = h->Pv;
    m.fr = h->frontier.as<int32_t>(); m.status = h->status.as<uint8_t>(); m.ctr = h->ctr.as<LevelCounters>(); m.dcnt = h->dcnt.as<int32_t>();
    m.theta_list = h->theta_list.as<int32_t>(); m.retry_list = h->retry_list.as<int32_t>(); m.part_lists = h->part_lists.as<int32_t>();
    m.targs = h->targs;
    m.zero[m.n_zero++] = {h->ctr.p, sizeof(LevelCounters)};
    m.zero[m.n_zero++] = {h->dcnt.p, DCNT_BYTES};
    m.use_kkt = small_kkt_on(h, m.kd, BATCH_KKT_THREAD_MAX, h->kn.no_kkt_thread == 1) ? 1 : 0;   // (MPC_NO_KKT_THREAD=2 switches off level_run_small's alone)
    if (m.use_kkt && h->kn.kkt_spread > 0 && m.kd <= BATCH_KKT_SPREAD_KMAX) m.use_kkt = 2;   // BATCH_KKT_SPREAD lanes per candidate (k_kkt_thread)
    m.kkt_listed = 0;
    if (m.use_kkt) {
        bool listed = false;
        { int rcb = small_kkt_buffers(h, nn, k, st, m.dcnt, m.targs, listed); if (rcb) return rcb; }
        m.kkt_code = h->kkt_code.as<uint8_t>(); m.kkt_L = h->kkt_L.as<double>();
        m.kkt_listed = listed ? 1 : 0;
    }
    // region stage: one slot per optimal candidate, buffers sized by the bound
    {
        int ldk = 0;
        { int rcb = small_region_slots(h, nn, st, ldk); if (rcb) return rcb; }
        m.zero[m.n_zero++] = {h->done_g.p, nn * 2 * sizeof(unsigned int)};
        m.rs.n_opt_dev = m.dcnt + DC_BATCH_OPT;   // the region launch comes last in the batch form: all optimal candidates
        m.rs.w_cap = h->grid_r2; m.rs.w_max = h->kn.rsplit_max;
        m.W = h->kn.no_rsplit ? 1 : 0;
        m.ldk = ldk; m.fd = h->fd; m.fi = h->fi; m.no_rbox = h->kn.no_rbox ? 1 : 0;
        m.headd = h->headd.as<double>(); m.headi = h->headi.as<int32_t>(); m.epool = h->epool.as<double>();
        m.kept_g = h->kept_g.as<uint8_t>(); m.done_g = h->done_g.as<unsigned int>();
        // retry slots of the LDS-engine region kernel (launch_region_v1's buffers)
        const int rows_t_ = h->n_c - h->n_eq + h->n_tc;
        m.rcap = (int)std::min<long long>(n, 256);
        HIP_TRY(h, h->recd.ensure((size_t)m.rcap * h->rec_d * sizeof(double), st));
        HIP_TRY(h, h->reci.ensure((size_t)m.rcap * h->rec_i * sizeof(int32_t), st));
        HIP_TRY(h, h->facet_flags.ensure((size_t)m.rcap * rows_t_, st));
        m.recd = h->recd.as<double>(); m.reci = h->reci.as<int32_t>(); m.facet_flags = h->facet_flags.as<uint8_t>();
        m.rec_d = h->rec_d; m.rec_i = h->rec_i; m.Pr = h->Pr; m.lds_r = h->lds_r;
    }
    // (x,theta) stage with the dictionary cache
    m.nxc = dict_nxc(h);
    DictCache dc;
    { int rcb = small_dict_cache(h, nn, gen_children, st, m.dcnt, dc); if (rcb) return rcb; }
    if (h->storing) m.zero[m.n_zero++] = {h->dict_stored[h->dict_cur].p, nn};
    m.dc = dc;
    m.storing = h->storing ? 1 : 0;
    m.dict_stored_cur = h->storing ? h->dict_stored[h->dict_cur].as<uint8_t>() : nullptr;
    m.quick_test = (!h->storing && dc.parent_slot) ? 1 : 0;
    // pruned masks + children
    m.keep_lowdim = (flags & MPC_LEVEL_KEEP_LOWDIM) ? 1 : 0;
    m.theta_open = h->theta_open ? 1 : 0;
    m.pruned = h->pruned.as<unsigned long long>(); m.n_pruned = h->n_pruned;
    if (gen_children) {
        { int rcb = small_children_buffers(h, nn, k, st); if (rcb) return rcb; }
        m.childmask = h->childmask.as<unsigned long long>(); m.count = h->count.as<int32_t>(); m.offset = h->offset.as<int32_t>();
        m.children = h->children.as<int32_t>(); m.parent_slot_next = h->parent_slot_next.as<int32_t>();
    }
    m.pub_ctr = reinterpret_cast<unsigned int *>(h->tot_dev + 16);
    m.pub_cnt = reinterpret_cast<unsigned int *>(h->tot_dev + 16 + (int)(sizeof(LevelCounters) / 4));
    // pruned.ensure(..., keep) may have moved the list: the frontier and everything else above is read after this point only
    HIP_TRY(h, hipStreamSynchronize(st));   // whatever the member's own stream still had queued (frontier kernels, copies of a grown buffer)
    return MPC_OK;
}

static int batch_finish(mpc_handle *h, int32_t gen_children, const BatchMember &m, float ms_total, mpc_level_stats *stats, bool *fallback) {
    *fallback = false;
    LevelCounters host_ctr;
    const int32_t *cnt_host = small_read_counters(h, host_ctr);
    if (cnt_host[DC_BATCH_RRETRY] > m.rcap || h->kn.test_small_fallback) {
        // more candidates k_region2 gave up on than retry slots were reserved (never observed): the member repeats the level alone
        h->n_smallpath_fallback++;
        *fallback = true;
        return MPC_OK;
    }
    small_take_counts(h, gen_children, host_ctr, cnt_host, DC_BATCH_OPT);
    h->n_rretry = cnt_host[DC_BATCH_RRETRY];      // their records are in the fixed layout (recd / reci), listed in retry_list
    level_close(h, h->n);
    if (stats) {
        level_stats_small(h, host_ctr, cnt_host, m.use_kkt != 0, m.quick_test != 0, stats);
        stats->n_region_retry = h->n_rretry;
        stats->ms_total = ms_total;   // the batch's launches, first to last (shared by all members)
    }
    return MPC_OK;
}

}   // namespace
