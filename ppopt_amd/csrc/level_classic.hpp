// level_classic.hpp -- the classic path of one level (host code only, no kernels): what level_run_impl of mpcombi_hip.hip runs for every
// level that does not take the path without host round trips (level_run_small), i.e. every large level.  Included by mpcombi_hip.hip
// alone, below mpc_handle and the engine's helpers it calls (launch_scan, launch_region_v1, x1_join, stream_ready, dict_cache_begin,
// level_record_shape, part_spec, ...): the translation unit stays one.
//
// LevelRun is the level's context: it lives on level_run_impl's stack, is built once per level and owns nothing.  Its member functions
// are the level's stages, in the order level_run_impl calls them (DESIGN 3.1 has the map), and the helpers the stages share (compact,
// partition, the collected preparations, the region launch, the end of the level).  What a stage leaves for a later one is a member, and
// each member says who sets it and who reads it.  The order of the calls on each stream, and of the host's waits between them, is the
// behaviour of the path: a stage function keeps the order its code had inside level_run_impl.
#pragma once

namespace {   // (internal linkage: the library exports the C ABI and nothing of this)

struct LevelRun {
    // ---- per-level constants ----------------------------------------------------------------------------------------------------------
    mpc_handle *const h;            // the handle (set by the constructor, as the next eight)
    const int32_t gen_children;     // the level generates children (the next level's candidates)
    const int32_t flags;            // MPC_LEVEL_* of the call
    const long long n;              // candidates of the level
    const int k;                    // their cardinality
    const size_t nn;                // n as a size
    const hipStream_t st;           // the handle's main stream
    const bool small;               // n <= SMALL_LEVEL_N: compact / partition as single-block launches
    const int blocks256, nb1024;    // blocks of 256 / 1024 candidates
    LevelCounters *ctr = nullptr;   // set by begin: the level's counters on the device; read by every stage
    int32_t *dcnt = nullptr;        // set by begin: the device-resident list lengths (words named by DcntWord, batch_level.hpp); read by every stage
    int32_t *total = nullptr;       // set by begin: device alias of h->tot_host, valid on the host after the next synchronisation; read by compact, partition, queue_tail, region_stage
    // ---- what the statistics report (set by the stages, read by read_back and fill_stats) ------------------------------------------------
    LevelCounters host_ctr;         // set by read_back (zero on an empty level): the counters as published; read by fill_stats
    float ms[3] = {0, 0, 0};        // set by read_back: verdict / region / children times between ev[0..3]; read by fill_stats
    float kms[5] = {0, 0, 0, 0, 0}; // set by read_back: kernel times of kernel_timed[]; read by fill_stats
    bool kernel_timed[5] = {false, false, false, false, false};   // set by theta_stage [0], first_partition / x_stage [1], region2_launch [2], kkt_stage [3], quick_test [4]: kev[2i], kev[2i+1] were recorded; read by read_back
    long long n_x_items = 0;        // set by x_stage, corrected by read_back: work items of the (x,theta) stage; read by fill_stats
    long long n_theta_items = 0;    // set by theta_stage, corrected by read_back: work items of the theta stage; read by fill_stats
    long long n_xq_items = 0;       // set by quick_test, corrected by read_back: what the quick test was given; read by fill_stats
    bool xq_thread_timed = false;   // set by early_thread_pass, launch_plans, quick_test: kev[10], kev[11] were recorded; read by read_back
    bool xq_early_ran = false;      // set by early_thread_pass: the pass ran beside the theta stage; read by read_back, fill_stats
    bool x1_ran = false;            // set by launch_plans: the one-step plans ran; read by read_back, fill_stats
    // ---- state the helpers share ------------------------------------------------------------------------------------------------------------
    bool pruned_bucketed = false;   // set by begin: the pruned list was bucketed for this level; read by queue_tail
    bool theta_lean = false;        // set by kkt_stage: the theta list's length stays on the device (DC_THETA); read by theta_stage, read_back
    bool xq_lean = false;           // set by quick_test: the length of what it left open stays on the device (DC_OPEN_QT); read by launch_x, x_stage, read_back
    bool children_lean = false;     // set by queue_tail: children written for the bound, their number in DC_CHILDREN; read by read_back
    // clears / copies / slot marks that a region launch and the (x,theta) stage need, collected and issued as ONE launch each
    // (k_region_prep): `prep` for the main stream, `rprep` for what only the region kernel reads (issued on ITS stream)
    RegionPrep prep{}, rprep{};     // set by prep_zero_in, overlapped_region_launch, retry_and_late, region2_launch; issued and cleared by prep_flush_on
    bool prep_any = false, rprep_any = false;   // set with prep / rprep: something is queued in them; read by prep_flush_on, read_back
    const uint8_t *kkc = nullptr;   // set by kkt_stage: KKT codes and multipliers of k_kkt_thread (read by k_theta2 / k_region2); read by early_thread_pass, theta_stage, region2_launch
    const double *kkl = nullptr;    // set by kkt_stage, with kkc
    int32_t *region_out_hi = nullptr;   // set by region2_launch: head_i of the level's slots as the device sees it (device buffer or mapped host block); read by retry_and_late
    bool region_launched = false;   // set by overlapped_region_launch, retry_and_late: the region kernel is on stream3; read by second_partition_and_tail, retry_and_late, region_stage
    int32_t n_late = 0;             // set by retry_and_late: optimal candidates found after an overlapped region launch (spare slots); read by region_stage
    int32_t n_opt_fast = -1;        // set by retry_and_late: >= 0: the fast path has already built h->opt_list; read by region_stage
    bool tail_done = false;         // set by second_partition_and_tail: the speculative end of the level stands; read by region_stage, tail
    // ---- the register-engine path (h->fast && !h->kn.force_v1), stage to stage -------------------------------------------------------------
    const int32_t *fr = nullptr;    // set by kkt_stage: the frontier; read by every later stage of the path
    uint8_t *stp = nullptr;         // set by kkt_stage: the status array; read by every later stage of the path
    const DevProblem *pf = nullptr; // set by kkt_stage: k_verdict2's view of the program on the device; read by every later stage of the path
    long long n_theta;              // set by the constructor (n), by kkt_stage (the bound): items of the theta stage; read by theta_stage
    const int32_t *theta_list = nullptr;   // set by kkt_stage: the theta stage's work list (nullptr: every candidate); read by theta_stage
    bool kkt_listed = false;        // set by kkt_stage: k_kkt_thread listed its own output (theta_list, xq_list); read by early_thread_pass
    bool early_xq = false;          // set by early_thread_pass: the thread pass runs on stream2 beside the theta stage; read by first_partition, overlapped_region_launch, open_list, quick_test
    int nxc = 0;                    // set by first_partition: dictionary columns k_x2 keeps; read by launch_plans, quick_test
    DictCache dc{};                 // set by first_partition (dict_cache_begin, pre1 / pre2), open_list (pre lists and their lengths); read by launch_plans, quick_test, x_stage
    bool x_done = false;            // set by first_partition (x_first): the (x,theta) stage is already queued; read by doubtful_side_stream, x_stage
    int32_t cntA[PART_CLASSES] = {0, 0, 0, 0};   // set by first_partition, open_list ([3]): classes after the theta stage; read by doubtful_side_stream, overlapped_region_launch, open_list
    int32_t n_early = 0;            // set by doubtful_side_stream: doubtful candidates of the theta stage, re-solved on stream2; read by overlapped_region_launch, second_partition_and_tail
    int32_t region_extra = 0;       // set by overlapped_region_launch, retry_and_late: spare slots behind the region launch's; read by retry_and_late
    size_t lds_q = 0;               // set by overlapped_region_launch: LDS bytes of one dictionary record (grouped quick test); read by quick_test
    bool quick_test_on = false;     // set by overlapped_region_launch: the level ends with the quick test (last level, decisions only); read by quick_test
    bool use_grouped = false;       // set by overlapped_region_launch: ... in its form grouped by parent; read by quick_test
    int32_t n_needx = 0;            // set by open_list: candidates whose feasibility is open (after quick_test: the bound); read by quick_test, x_stage
    const int32_t *needx_list = nullptr;   // set by open_list, quick_test: their list; read by quick_test, x_stage
    int32_t cntB[PART_CLASSES] = {0, 0, 0, 0};   // set by second_partition_and_tail, retry_and_late: classes after the (x,theta) stage; read by retry_and_late
    bool have_cntB = false;         // set by second_partition_and_tail: cntB was read with the speculative end; read by retry_and_late

    LevelRun(mpc_handle *h_, int32_t gen_children_, int32_t flags_)
        : h(h_), gen_children(gen_children_), flags(flags_), n(h_->n), k(h_->k), nn((size_t)h_->n), st(h_->stream), small(h_->n <= SMALL_LEVEL_N),
          blocks256((int)((h_->n + 255) / 256)), nb1024((int)((h_->n + 1023) / 1024)), n_theta(h_->n) {
        std::memset(&host_ctr, 0, sizeof(host_ctr));
    }

    // ==== helpers ==========================================================================================================================
    int32_t *part_list(int c) const { return h->part_lists.as<int32_t>() + (size_t)c * nn; }

    // compacts the candidates whose status lies in [lo, hi] into h->retry_list; returns their number
    // count_dev != nullptr: the length goes to device memory only and nobody waits for it (the consumer kernel reads it there)
    int compact(int lo, int hi, int32_t *count, int32_t *count_dev = nullptr) {
        HIP_TRY(h, h->retry_list.ensure(nn * sizeof(int32_t), st));
        int32_t *tot = count_dev ? count_dev : total;
        if (small) {
            hipLaunchKernelGGL(k_compact_small, dim3(1), dim3(1024), 0, st, h->status.as<uint8_t>(), (int)n, lo, hi, h->retry_list.as<int32_t>(), tot);
        } else {
            hipLaunchKernelGGL(k_flag_status, dim3(blocks256), dim3(256), 0, st, h->status.as<uint8_t>(), n, lo, hi, h->flag.as<int32_t>());
            int rcs = launch_scan(h, h->flag.as<int32_t>(), h->pos.as<int32_t>(), n, tot);
            if (rcs) return rcs;
            hipLaunchKernelGGL(k_scatter_index, dim3(blocks256), dim3(256), 0, st, h->flag.as<int32_t>(), h->pos.as<int32_t>(), n, h->retry_list.as<int32_t>());
        }
        HIP_TRY(h, hipGetLastError());
        if (count_dev) return MPC_OK;
        HIP_TRY(h, hipStreamSynchronize(st));
        *count = h->tot_host[0];
        return MPC_OK;
    }

    // deterministic partition of the candidates into up to four lists by status (spec: status -> class nibble, 15 = none);
    // the lists are h->part_lists + c * n, their lengths come back in counts[]
    // deferred: the counts go to the pinned words [12..15] and nobody waits here (the caller reads them after a later synchronisation)
    int partition(std::initializer_list<std::pair<int, int>> classes, int32_t counts[PART_CLASSES], bool deferred = false, int32_t *tot_dev_mem = nullptr) {
        const unsigned long long spec = part_spec(classes);
        HIP_TRY(h, h->part_counts.ensure((size_t)PART_CLASSES * nb1024 * sizeof(int32_t), st));
        HIP_TRY(h, h->part_lists.ensure((size_t)PART_CLASSES * nn * sizeof(int32_t), st));
        int32_t *tot = tot_dev_mem ? tot_dev_mem : (deferred ? total + 12 : total);   // tot_dev_mem: the lengths stay in device memory (the caller publishes them)
        if (small) {
            hipLaunchKernelGGL(k_partition_small, dim3(1), dim3(1024), 0, st, h->status.as<uint8_t>(), (int)n, spec, h->part_lists.as<int32_t>(), (long long)n, tot);
        } else {
            hipLaunchKernelGGL(k_part_count, dim3(nb1024), dim3(1024 / SCAN_IT), 0, st, h->status.as<uint8_t>(), n, spec, h->part_counts.as<int32_t>(), nb1024);
            hipLaunchKernelGGL(k_part_sums, dim3(PART_CLASSES), dim3(1024 / SCAN_IT), 0, st, h->part_counts.as<int32_t>(), nb1024, tot);
            hipLaunchKernelGGL(k_part_scatter, dim3(nb1024), dim3(1024 / SCAN_IT), 0, st, h->status.as<uint8_t>(), n, spec, h->part_counts.as<int32_t>(), nb1024,
                               h->part_lists.as<int32_t>());
        }
        HIP_TRY(h, hipGetLastError());
        if (deferred) return MPC_OK;
        HIP_TRY(h, hipStreamSynchronize(st));
        for (int c = 0; c < PART_CLASSES; ++c) counts[c] = h->tot_host[c];
        return MPC_OK;
    }

    int prep_flush_on(RegionPrep &pp, bool &any, hipStream_t ps) {
        if (!any) return MPC_OK;
        unsigned long long work = (unsigned long long)std::max<long long>(pp.copy_n, pp.extra);
        for (int j = 0; j < 4; ++j) work = std::max(work, pp.z.bytes[j] / 8);
        hipLaunchKernelGGL(k_region_prep, dim3((unsigned)std::min<unsigned long long>(256, work / 1024 + 1)), dim3(256), 0, ps, pp);
        HIP_TRY(h, hipGetLastError());
        pp = RegionPrep{}; any = false;
        return MPC_OK;
    }
    int prep_flush() { return prep_flush_on(prep, prep_any, st); }
    int prep_zero_in(RegionPrep &pp, bool &any, hipStream_t ps, void *ptr, size_t bytes) {
        if (!ptr || bytes == 0) return MPC_OK;
        int j = 0;
        while (j < 4 && pp.z.p[j]) ++j;
        if (j == 4) { int rcs = prep_flush_on(pp, any, ps); if (rcs) return rcs; j = 0; }
        pp.z.p[j] = ptr; pp.z.bytes[j] = bytes; any = true;
        return MPC_OK;
    }
    int prep_zero(void *ptr, size_t bytes) { return prep_zero_in(prep, prep_any, st, ptr, bytes); }

    // The previous level's sets as the OTHER parents of this level's candidates (k_xq_thread): its frontier (it lives in the children buffer
    // since the hand-over) and its "dictionary stored" bytes, if both are still there; `tries`: most other parents the kernel asks per
    // candidate.  Whether a pass looks at other parents at all is its caller's own switch.
    XqAlt other_parents(int tries) const {
        XqAlt alt{};
        if (h->n_prev > 0 && h->n_prev <= 0x7fffffffLL && k >= 2 &&
            h->children.cap >= (size_t)h->n_prev * (k - 1) * sizeof(int32_t) && h->dict_stored[1 - h->dict_cur].cap >= (size_t)h->n_prev) {
            alt.prev_frontier = h->children.as<int32_t>(); alt.prev_stored = h->dict_stored[1 - h->dict_cur].as<uint8_t>();
            alt.n_prev = (int)h->n_prev; alt.tries = tries;   // (the kernel stops at the candidate's inequality members)
        }
        return alt;
    }

    // region stage on the register engine: one slot per candidate of h->opt_ptr.  Buffers are prepared on the main stream; the
    // kernel goes to `rst` (the main stream, or stream3 when the stage runs under the level's (x,theta) stage)
    int region2_launch(int32_t n_opt, int32_t extra, hipStream_t rst, bool one_wave) {
        const int rows_t_ = h->n_c - h->n_eq + h->n_tc;
        const size_t n_tot = (size_t)n_opt + (size_t)extra;   // slots: the launch's candidates + spare ones for late optimal candidates
        HIP_TRY(h, h->headd.ensure(n_tot * h->fd * sizeof(double), st));
        HIP_TRY(h, h->headi.ensure(n_tot * h->fi * sizeof(int32_t), st));
        HIP_TRY(h, h->epool.ensure(n_tot * rows_t_ * (h->n_t + 1) * sizeof(double), st));
        // few optimal candidates: several wavefronts per candidate (the facet tests are split among them)
        int W = (h->kn.no_rsplit || one_wave) ? 1 : h->kn.rsplit_max;
        while (W > 1 && (long long)n_opt * W > h->grid_r2) W >>= 1;
        const int ldk = (rows_t_ + 1 + 63) & ~63;
        if (W > 1) {
            HIP_TRY(h, h->kept_g.ensure((size_t)n_opt * ldk, st));
            HIP_TRY(h, h->done_g.ensure((size_t)n_opt * 2 * sizeof(unsigned int), st));
            { int rcs = prep_zero_in(rprep, rprep_any, rst, h->done_g.p, (size_t)n_opt * 2 * sizeof(unsigned int)); if (rcs) return rcs; }
        }
        // an overlapped launch may take only a share of the wave slots (r2_cap_pct): its 256-register wavefronts otherwise fill the
        // register file of every SIMD they sit on and the (x,theta) kernel beside them gets no slot there until they leave
        const long long grid_cap = (rst != st && one_wave) ? std::max<long long>(h->n_cu, (long long)h->grid_r2 * h->kn.r2_cap_pct / 100) : h->grid_r2;
        const dim3 g((unsigned)std::min<long long>((long long)n_opt * W, grid_cap));
        const DevProblem *pr = h->pr2_dev.as<DevProblem>();
        // where the records go: device buffers (fetched / gathered later), or -- streaming -- page-locked host blocks the
        // kernel writes directly, in chunks the host consumes while the kernel is still running
        double *out_hd = h->headd.as<double>(), *out_er = h->epool.as<double>();
        int32_t *out_hi = h->headi.as<int32_t>();
        RegionStream rs{};
        const size_t bytes_hd = n_tot * h->fd * sizeof(double), bytes_hi = n_tot * h->fi * sizeof(int32_t),
                     bytes_er = n_tot * rows_t_ * (h->n_t + 1) * sizeof(double);
        if ((flags & MPC_LEVEL_STREAM) && bytes_hd + bytes_hi + bytes_er <= (size_t(1) << 30)) {
            auto &so = h->so;
            so.shift = 8;
            while (so.shift > 4 && ((long long)n_opt >> so.shift) < 8) --so.shift;   // at least ~8 chunks, 16..256 slots each
            so.n_chunks = (int)(((long long)n_opt + (1ll << so.shift) - 1) >> so.shift);
            so.n_slots = (long long)n_tot; so.cap_rows = (long long)n_tot * rows_t_;   // chunks cover the first n_opt slots
            HIP_TRY(h, host_pool_take(bytes_hd, &so.hd, nullptr, true));
            HIP_TRY(h, host_pool_take(bytes_hi, &so.hi, nullptr, true));
            HIP_TRY(h, host_pool_take(std::max<size_t>(bytes_er, 8), &so.er, nullptr, true));
            h->st_flags.coherent = true;
            HIP_TRY(h, h->st_flags.ensure((size_t)so.n_chunks * sizeof(int32_t)));
            std::memset(h->st_flags.p, 0, (size_t)so.n_chunks * sizeof(int32_t));
            h->cw_chunks = so.n_chunks;
            HIP_TRY(h, h->chunk_count.ensure((size_t)so.n_chunks * sizeof(unsigned int), st));
            { int rcs = prep_zero_in(rprep, rprep_any, rst, h->chunk_count.p, (size_t)so.n_chunks * sizeof(unsigned int)); if (rcs) return rcs; }
            void *d_hd = nullptr, *d_hi = nullptr, *d_er = nullptr, *d_fl = nullptr;
            HIP_TRY(h, hipHostGetDevicePointer(&d_hd, so.hd, 0));
            HIP_TRY(h, hipHostGetDevicePointer(&d_hi, so.hi, 0));
            HIP_TRY(h, hipHostGetDevicePointer(&d_er, so.er, 0));
            HIP_TRY(h, hipHostGetDevicePointer(&d_fl, h->st_flags.p, 0));
            out_hd = static_cast<double *>(d_hd); out_hi = static_cast<int32_t *>(d_hi); out_er = static_cast<double *>(d_er);
            rs.count = h->chunk_count.as<unsigned int>(); rs.flags = static_cast<int32_t *>(d_fl); rs.shift = so.shift; rs.n_slots = n_opt;
            so.active = true;
        }
        region_out_hi = out_hi;
        if (extra > 0) { rprep.head_i = out_hi; rprep.fi = h->fi; rprep.first = n_opt; rprep.extra = extra; rprep_any = true; }
        if (rst != st) {
            // The side stream does NOT wait for the main stream: every caller has synchronised the main stream (the partition whose
            // counts sized this launch) and has queued nothing since that the region kernel reads, so the region stage's own
            // preparation and the kernel go straight to the side stream -- one cross-stream hop (~25 us) less per large level than the
            // fork through an event.  The main stream continues only when the side stream has reached the region kernel, so that
            // the region wavefronts (the long chains) are placed first and the (x,theta) kernels fill in around them -- without this
            // the two dispatches race and the persistent (x,theta) kernel often takes the whole GPU first.
            { int rcs = prep_flush_on(rprep, rprep_any, rst); if (rcs) return rcs; }
            HIP_TRY(h, hipEventRecord(h->ev_rgo, rst));
            HIP_TRY(h, hipStreamWaitEvent(st, h->ev_rgo, 0));
        } else {
            { int rcs = prep_flush(); if (rcs) return rcs; }
            { int rcs = prep_flush_on(rprep, rprep_any, st); if (rcs) return rcs; }
        }
        if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[4], rst));
        const int nt_r = region2_nt(h->fast_r);
        launch_region2(h->fast_r, g, h->lds_r2, rst, pr, h->frontier.as<int32_t>(), k, h->opt_ptr, n_opt, h->status.as<uint8_t>(), out_hd, out_hi, h->fd, h->fi, out_er,
                       ctr, kkc, kkl, W, h->kept_g.as<uint8_t>(), ldk, h->done_g.as<unsigned int>(),
                       h->kn.no_rbox ? (const double *)nullptr : h->targs.tvp + (size_t)nt_r * nt_r + nt_r, rs);
        if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[5], rst));
        if (rst != st) { h->r3_dirty = true; h->region_side_stream = true; HIP_TRY(h, hipEventRecord(h->ev_rjoin, rst)); }
        kernel_timed[2] = true;
        HIP_TRY(h, hipGetLastError());
        h->used_region2 = true;
        stream_ready(h);   // the caller of mpc_level_stream_info may start consuming chunks
        return MPC_OK;
    }

    // The end of a level -- pruned masks, children, histogram, counters published -- as launches only (the caller synchronises).
    int queue_tail() {
        const int keep_lowdim = (flags & MPC_LEVEL_KEEP_LOWDIM) ? 1 : 0;
        if (flags & MPC_LEVEL_GRAPH) { /* no pruning in the graph traversal */ }
        else launch_pruned_append(h->mw, dim3(blocks256), st, h->frontier.as<int32_t>(), n, k, h->status.as<uint8_t>(),
                                  h->pruned.as<unsigned long long>() + (size_t)h->n_pruned * h->mw, ctr, keep_lowdim);
        if (gen_children) {
            HIP_TRY(h, h->childmask.ensure(nn * h->mw * sizeof(uint64_t), st));
            HIP_TRY(h, h->count.ensure(nn * sizeof(int32_t), st));
            HIP_TRY(h, h->offset.ensure(nn * sizeof(int32_t), st));
            if (pruned_bucketed)
                launch_children_count_b(h->mw, dim3((unsigned)n), st, h->Pv, h->frontier.as<int32_t>(), n, k, h->status.as<uint8_t>(),
                                        h->pruned_b.as<unsigned long long>(), h->pruned_head.as<int32_t>(), h->childmask.as<unsigned long long>(), h->count.as<int32_t>(), keep_lowdim);
            else
                launch_children_count(h->mw, dim3((unsigned)n), st, h->Pv, h->frontier.as<int32_t>(), n, k, h->status.as<uint8_t>(),
                                      h->pruned.as<unsigned long long>(), (long long)h->n_pruned, h->childmask.as<unsigned long long>(), h->count.as<int32_t>(), keep_lowdim);
            // lean: children and their parent slots are sized by the bound n (n_c - k) and written without waiting for the count
            const double child_bound_bytes = (double)nn * std::max(h->n_c - k, 1) * (k + 2) * 4.0;
            children_lean = child_bound_bytes <= 1.5e9;
            { int rcs = launch_scan(h, h->count.as<int32_t>(), h->offset.as<int32_t>(), n, children_lean ? dcnt + DC_CHILDREN : total); if (rcs) return rcs; }
            HIP_TRY(h, hipGetLastError());
            int32_t n_children = 0;
            if (children_lean) n_children = (int32_t)std::min<double>((double)nn * std::max(h->n_c - k, 1), 2147483647.0 / (k + 2));   // the bound, for the allocation only
            else { HIP_TRY(h, hipStreamSynchronize(st)); n_children = h->tot_host[0]; }
            h->n_children = children_lean ? 0 : n_children;
            if (n_children > 0) {
                HIP_TRY(h, h->children.ensure((size_t)n_children * (k + 1) * sizeof(int32_t), st));
                HIP_TRY(h, h->parent_slot_next.ensure((size_t)n_children * sizeof(int32_t), st));
                { int rcj = defer_join(h, st); if (rcj) return rcj; }   // the children buffer is the frontier a deferred region launch of the small level before reads
                hipLaunchKernelGGL(k_children_write, dim3((unsigned)n), dim3(64), 0, st, h->frontier.as<int32_t>(), n, k, h->mw,
                                   h->childmask.as<unsigned long long>(), h->offset.as<int32_t>(), h->children.as<int32_t>(),
                                   h->storing ? h->dict_stored[h->dict_cur].as<uint8_t>() : (const uint8_t *)nullptr, h->parent_slot_next.as<int32_t>());
                HIP_TRY(h, hipGetLastError());
            }
        }
        hipLaunchKernelGGL(k_histogram, dim3(std::min(blocks256, 1024)), dim3(256), 0, st, h->status.as<uint8_t>(), n, ctr);
        HIP_TRY(h, hipGetLastError());
        if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[3], st));
        hipLaunchKernelGGL(k_publish_words2, dim3(1), dim3(128), 0, st, reinterpret_cast<const unsigned int *>(ctr), (int)(sizeof(LevelCounters) / 4),
                           reinterpret_cast<const unsigned int *>(dcnt), DCNT_WORDS, reinterpret_cast<unsigned int *>(h->tot_dev + 16));
        HIP_TRY(h, hipGetLastError());
        return MPC_OK;
    }

    // open parameter set: the candidates the verdict stage calls optimal are asked whether the reference's max-t LP is bounded (k_recession)
    int recession() {
        if (!h->theta_open || (flags & MPC_LEVEL_GRAPH)) return MPC_OK;
        hipLaunchKernelGGL(k_recession, dim3((unsigned)std::min<long long>(n, h->grid_v)), dim3(64), h->lds_v, st, h->Pv, h->frontier.as<int32_t>(), n, k, h->status.as<uint8_t>());
        HIP_TRY(h, hipGetLastError());
        return MPC_OK;
    }

    // The (x,theta) stage of a level that keeps dictionaries, in its one-step-plan form, needs no count from the host: its lists
    // come from the partition below, their lengths stay in device memory (DC_XFIRST_CLASS and the three words behind it), its launches are sized by the bound n.
    // Round 5 (`x_first`): it is queued BEHIND THE PARTITION AT ONCE, and only then does the host wait for the counts that size
    // the region stage -- until then the stage waited ~0.1 ms per large level for that read-back and the region launch's host work
    // (tools/timeline.sh: 110 us between the partition and the plan pass on level 4 of config 4).
    int launch_plans(const int32_t *needx_list_, int n_needx_, long long n_bound, const int32_t *n_needx_dev, const int32_t *n_pre1_dev, const int32_t *n_pre2_dev) {
        // One-step plans (round 5).  Every candidate that needs a dictionary is asked by ONE THREAD whether a parent's record is
        // one known step away (k_xq_thread in plan mode: the generating parent, then the candidate's other parents); k_x1 then
        // streams that record through the step -- no tableau in registers, no pricing, no ratio test --, and only what has no
        // such plan goes through the register simplex k_x2 as before, from its generating parent.
        { int rcq = prep_flush(); if (rcq) return rcq; }
        HIP_TRY(h, h->x1_buf.ensure((6 * nn + 16) * sizeof(int32_t), st));
        int32_t *xb = h->x1_buf.as<int32_t>();
        XqPlan pl{};
        pl.plan_slot = xb; pl.plan_step = xb + nn; pl.x1_list = xb + 2 * nn; pl.x1_n = dcnt + DC_X1;
        for (int sg = 0; sg < 3; ++sg) { pl.rest[sg] = xb + (3 + sg) * nn; pl.rest_n[sg] = dcnt + DC_X1_REST + sg; }
        pl.pre1 = dc.pre1; pl.n_pre1 = dc.n_pre1; pl.pre2 = dc.pre2; pl.n_pre2 = dc.n_pre2;
        pl.n_pre1_dev = n_pre1_dev; pl.n_pre2_dev = n_pre2_dev;
        XqAlt alt{};
        if (h->kn.x1 >= 2) alt = other_parents(MPC_MAX_NC);
        DictCache dq = dc;
        dq.n_list_dev = n_needx_dev;
        const DevProblem *pfx = h->pf_dev.as<DevProblem>();
        const int32_t *frx = h->frontier.as<int32_t>();
        uint8_t *stx = h->status.as<uint8_t>();
        const unsigned gt = (unsigned)std::min<long long>((n_bound + 63) / 64, (long long)h->n_cu * h->kn.xqt_wpc);
        if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[10], st));
        hipLaunchKernelGGL(k_xq_thread, dim3(gt), dim3(64), 0, st, pfx, frx, k, needx_list_, n_needx_, stx, ctr, dq, nxc, alt, pl);
        if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[11], st));
        xq_thread_timed = true;
        const unsigned g1 = (unsigned)std::min<long long>(n_bound, (long long)h->n_cu * h->kn.x1_wpc);
        // Round 6: the stream of one-step dictionaries goes to stream4 and is NOT waited for by this level: its records are read
        // by the next level's (x,theta) kernels only (x1_join), the plan pass has already marked the planned candidates as
        // "dictionary stored" for k_children_write.  The end of this level (k_x2 for the unplanned rest, children, counters), the
        // hand-over and the next level's KKT kernel run beside it.
        const bool defer = h->kn.x1_defer > 0 && !h->timing && h->stream4;
        hipStream_t sx1 = defer ? h->stream4 : st;
        if (defer) { HIP_TRY(h, hipEventRecord(h->ev_x1go, st)); HIP_TRY(h, hipStreamWaitEvent(sx1, h->ev_x1go, 0)); }
        if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[12], st));
        LevelCounters *ctr_x1 = defer ? (LevelCounters *)nullptr : ctr;   // (its pivot count would land in the next level's counters)
        launch_x1(h->fast_x, dim3(g1), sx1, pfx, pl.x1_list, pl.x1_n, ctr_x1, dc, nxc, pl.plan_slot, pl.plan_step);
        HIP_TRY(h, hipGetLastError());
        if (defer) { HIP_TRY(h, hipEventRecord(h->ev_x1done, sx1)); h->x1_pending = true; }
        if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[13], st));
        // what is left: the register simplex, list lengths on the device
        DictCache dr = dc;
        dr.pre1 = pl.rest[0]; dr.n_pre1 = 0; dr.n_pre1_dev = pl.rest_n[0];
        dr.pre2 = pl.rest[1]; dr.n_pre2 = 0; dr.n_pre2_dev = pl.rest_n[1];
        dr.n_list_dev = pl.rest_n[2]; dr.chunk = 0;
        const long long grid_r = (long long)h->n_cu * std::min<long long>(4, h->kn.x2_wpc);
        launch_x2(h->fast_x, dim3((unsigned)std::max<long long>(1, std::min<long long>(n_bound, grid_r))), st, pfx, frx, k, pl.rest[2], n_needx_, stx, ctr, dr);
        HIP_TRY(h, hipGetLastError());
        x1_ran = true;
        return MPC_OK;
    }

    int launch_x(const int32_t *ls, int n_items, const DictCache &d0) {
        // ctr->work_x is zero: the counters were cleared at the start of the level and this is the level's only k_x2 launch
        { int rcs = prep_flush(); if (rcs) return rcs; }
        DictCache d = d0;
        // wavefronts per CU of the persistent launch: fewer for fewer items (an item is faster the fewer wavefronts share its SIMD; round 4,
        // config 4: level 3, 15.7 k items, 0.445 ms with 16 per CU, 0.33 with 4; level 4, 138 k items, 1.134 / 1.083 / 1.161 ms with 16 / 12 / 8)
        const long long n_all = (long long)n_items + d.n_pre1 + d.n_pre2;
        const long long wpc = std::max<long long>(std::min<long long>(4, h->kn.x2_wpc), std::min<long long>(h->kn.x2_wpc, n_all / ((long long)h->kn.x2_div * h->n_cu)));
        const long long grid_x = (long long)h->n_cu * wpc;
        d.chunk = (int)std::max<long long>(1, std::min<long long>(16, n_all / (grid_x * 8)));
        if (xq_lean) { d.n_list_dev = dcnt + DC_OPEN_QT; d.chunk = 0; }   // length of `ls` and chunk rule on the device
        launch_x2(h->fast_x, dim3((unsigned)std::min<long long>(xq_lean ? n_all : (n_all + d.chunk - 1) / d.chunk, grid_x)), st, pf, fr, k, ls, n_items, stp, ctr, d);
        HIP_TRY(h, hipGetLastError());
        return MPC_OK;
    }

    // ==== stages, in the order of the level ====================================================================================================
    // buffers sized by the number of candidates, counters and list lengths cleared, the pruned list bucketed; ends with the level's first event
    int begin() {
        HIP_TRY(h, h->status.ensure(nn, st));
        HIP_TRY(h, h->flag.ensure(nn * sizeof(int32_t), st));
        HIP_TRY(h, h->pos.ensure(nn * sizeof(int32_t), st));
        HIP_TRY(h, h->opt_list.ensure(nn * sizeof(int32_t), st));
        HIP_TRY(h, h->pruned.ensure((size_t)(h->n_pruned + n) * h->mw * sizeof(uint64_t), st, true));   // the level's newly pruned masks go behind the list
        ctr = h->ctr.as<LevelCounters>();
        total = h->tot_dev;          // device alias of h->tot_host: valid on the host after the next synchronisation
        // Lean form of a large level (round 3): the classic sequence read a list length back after almost every stage -- 22 idle gaps of
        // 15-30 us per solve of config 4 (tools/gpu_idle.sh).  The host needs only the lengths that size the region stage (one
        // read-back after the theta stage) and the final statistics; the theta LP, the (x,theta) stage after the quick test and the
        // child generation take theirs from device memory (dcnt: DC_THETA, DC_OPEN_QT, DC_CHILDREN) and are
        // launched for the bound the host does know.
        HIP_TRY(h, h->dcnt.ensure(DCNT_BYTES, st));
        {   // counters and list lengths cleared by one launch (a hipMemsetAsync costs the host ~16 us, a launch ~3 us)
            ZeroBufs z{};
            z.p[0] = h->ctr.p; z.bytes[0] = sizeof(LevelCounters);
            z.p[1] = h->dcnt.p; z.bytes[1] = DCNT_BYTES;
            hipLaunchKernelGGL(k_zero_bufs, dim3(1), dim3(256), 0, st, z);
            HIP_TRY(h, hipGetLastError());
        }
        // (round 6) the pruned list of the earlier levels, bucketed by smallest non-equality member, for this level's children stage: three
        // small launches at the level's start (nothing waits for them before k_children_count_b)
        if (gen_children && !(flags & MPC_LEVEL_GRAPH) && h->kn.pruned_bucket_min > 0 && h->n_c <= 256 && h->n_pruned >= std::max<long long>(1, h->kn.pruned_bucket_np) &&
            (double)n * (double)h->n_pruned >= h->kn.pruned_bucket_min && h->n_pruned <= 0x7fffffffLL) {
            HIP_TRY(h, h->pruned_b.ensure((size_t)h->n_pruned * h->mw * sizeof(uint64_t), st));
            HIP_TRY(h, h->pruned_head.ensure((size_t)PB_WORDS * sizeof(int32_t), st));
            HIP_TRY(h, hipMemsetAsync(h->pruned_head.p, 0, (size_t)PB_WORDS * sizeof(int32_t), st));
            const dim3 gb((unsigned)((h->n_pruned + 255) / 256));
            const int ne_b = h->n_eq;
            launch_pruned_bucket_count(h->mw, gb, st, h->pruned.as<unsigned long long>(), (long long)h->n_pruned, ne_b, h->pruned_head.as<int32_t>());
            hipLaunchKernelGGL(k_pruned_bucket_scan, dim3(1), dim3(256), 0, st, h->pruned_head.as<int32_t>());
            launch_pruned_bucket_scatter(h->mw, gb, st, h->pruned.as<unsigned long long>(), (long long)h->n_pruned, ne_b, h->pruned_head.as<int32_t>(), h->pruned_b.as<unsigned long long>());
            HIP_TRY(h, hipGetLastError());
            pruned_bucketed = true;
        }
        dcnt = h->dcnt.as<int32_t>();
        level_record_shape(h, k);
        // verdict
        if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[0], st));
        return MPC_OK;
    }

    // KKT solves + box screen, one thread per candidate (Schur/Cholesky mode, cardinality 1..8); the wave kernels
    // fetch the multipliers of the candidates the screen left open
    int kkt_stage() {
        fr = h->frontier.as<int32_t>();
        stp = h->status.as<uint8_t>();
        pf = h->pf_dev.as<DevProblem>();
        const int kd = k - h->targs.ne;   // rows the one-thread KKT kernel solves for (the equality rows are eliminated)
        if (h->kkt_mode == 0 && kd >= 1 && kd <= KKT_THREAD_MAX && h->kn.no_kkt_thread != 1) {
            HIP_TRY(h, h->kkt_code.ensure(nn, st));
            HIP_TRY(h, h->kkt_L.ensure(nn * (size_t)k * (h->n_t + 1) * sizeof(double), st));
            kkc = h->kkt_code.as<uint8_t>(); kkl = h->kkt_L.as<double>();
            // (round 6) KKT_SPREAD lanes per candidate while that still leaves the level short of the chip's thread slots (k_kkt_thread's comment)
            const bool spread = h->kn.kkt_spread > 0 && kd <= KKT_SPREAD_KMAX && n * KKT_SPREAD <= (long long)h->kn.kkt_spread_threads;
            const dim3 g((unsigned)(spread ? (n * KKT_SPREAD + 255) / 256 : blocks256));
            ThetaArgs ta = h->targs;
            // (round 5) the kernel lists its own output: the theta stage's work list and the candidates its box screen sends to
            // the (x,theta) question -- two compactions of five launches each saved on the level's critical path
            const bool kkt_lists = !h->kn.no_kkt_lists && n <= 0x7fffffffLL;
            if (kkt_lists) {
                HIP_TRY(h, h->theta_list.ensure(nn * sizeof(int32_t), st));
                HIP_TRY(h, h->xq_list.ensure(nn * sizeof(int32_t), st));
                ta.kt_list = h->theta_list.as<int32_t>(); ta.kt_n = dcnt + DC_THETA;
                ta.kx_list = h->xq_list.as<int32_t>(); ta.kx_n = dcnt + DC_KX;
            }
            if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[6], st));
            launch_kkt_thread(kd, h->fast_t, spread, g, st, pf, fr, n, h->kkt_code.as<uint8_t>(), h->kkt_L.as<double>(), stp, ta, ctr);
            if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[7], st));
            kernel_timed[3] = true;
            HIP_TRY(h, hipGetLastError());
            if (kkt_lists) kkt_listed = true;
            else {
                { int rcs = compact(ST_TODO, ST_TODO, nullptr, dcnt + DC_THETA); if (rcs) return rcs; }
                HIP_TRY(h, h->theta_list.ensure(nn * sizeof(int32_t), st));
                std::swap(h->theta_list, h->retry_list);   // compact() filled retry_list; keep it as the theta list
            }
            theta_lean = true;
            n_theta = (int32_t)n;   // the bound
            theta_list = h->theta_list.as<int32_t>();
        }
        return MPC_OK;
    }

    // The quick test's thread pass BESIDE the theta stage (round 5).  On a level that keeps no dictionaries, k_kkt_thread's box
    // screen has already sent almost every candidate to the (x,theta) question (config 4's last level: 98.5 %), and that
    // question does not depend on the theta stage at all.  Their list is cut here and k_xq_thread takes it on the second
    // stream -- a kernel bound by the cache's request rate beside one bound by dependent fp64 latency -- ; the two meet
    // before the partition that follows the theta stage, which then sees only what the pass left open.
    // (the previous level's deferred k_x1 is joined by whoever reads dictionary records first: the thread pass on the second stream
    //  below -- the theta kernel reads none and goes ahead --, else the (x,theta) stage behind the theta stage)
    int early_thread_pass() {
        if (kkc && h->kn.xq_thread != 0 && !(flags & MPC_LEVEL_GRAPH) && h->have_prev_dict && h->have_parent_slot &&
            n >= h->kn.xqt_min && (h->prev_regions < h->kn.xq_early_regions || h->kn.xq_early_regions <= 0)) {
            // (The pass then overlaps the theta stage AND the region stage: the partition behind the theta stage lists only the doubtful
            //  and the optimal candidates -- classes the pass never touches --, the region kernel starts on its stream, and the open
            //  candidates are listed when the pass has ended.  Config 4's last level: 1.86 ms with the pass behind the theta stage,
            //  1.72 beside it; config 3's: 3.45 / 3.25.)
            const int nxc_e = dict_nxc(h);
            const long long sd_e = (long long)nxc_e * h->Pf.n_d0r, si_e = dict_ints(h->Pf.n_d0r, nxc_e, h->n_c);
            if (!dict_will_store(h, nn, gen_children)) {
                if (!kkt_listed) {      // (else k_kkt_thread has listed them in xq_list, length in DC_KX)
                    { int rcs = compact(ST_NEEDX, ST_NEEDX_SING, nullptr, dcnt + DC_KX); if (rcs) return rcs; }
                    HIP_TRY(h, h->xq_list.ensure(nn * sizeof(int32_t), st));
                    std::swap(h->xq_list, h->retry_list);
                }
                DictCache dq{};
                dq.stride_d = sd_e; dq.stride_i = si_e;
                dq.parent_slot = h->parent_slot.as<int32_t>();
                dq.prev_d = h->dict_d[1 - h->dict_cur].as<double>(); dq.prev_i = h->dict_i[1 - h->dict_cur].as<int32_t>();
                dq.n_list_dev = dcnt + DC_KX;
                XqAlt alt{};
                if (h->kn.xq_thread >= 2 || h->kn.xq_thread < 0) alt = other_parents(h->kn.xq_thread < 0 ? MPC_MAX_NC : h->kn.xq_thread - 1);
                HIP_TRY(h, hipEventRecord(h->ev_xfork, st));
                HIP_TRY(h, hipStreamWaitEvent(h->stream2, h->ev_xfork, 0));
                if (h->x1_pending) HIP_TRY(h, hipStreamWaitEvent(h->stream2, h->ev_x1done, 0));   // (the main stream joins later: x1_join before its own first reader)
                const unsigned gt = (unsigned)std::min<long long>((n + 63) / 64, (long long)h->n_cu * h->kn.xqt_wpc);
                if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[10], h->stream2));
                hipLaunchKernelGGL(k_xq_thread, dim3(gt), dim3(64), 0, h->stream2, pf, fr, k, h->xq_list.as<int32_t>(), (int)n, stp, ctr, dq, nxc_e, alt, XqPlan{});
                if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[11], h->stream2));
                HIP_TRY(h, hipGetLastError());
                HIP_TRY(h, hipEventRecord(h->ev_xjoin, h->stream2));
                xq_thread_timed = true;
                early_xq = true; xq_early_ran = true;
            }
        }
        return MPC_OK;
    }

    int theta_stage() {
        if (n_theta > 0) {   // two-stage theta LP
            ThetaArgs ta = h->targs;
            ta.chunk = (int)std::max<long long>(1, std::min<long long>(16, n_theta / ((long long)h->grid_f * 8)));
            if (theta_lean) { ta.n_dev = dcnt + DC_THETA; ta.chunk = 0; }   // length and chunk rule on the device
            // wave slots the theta kernel takes (ThetaArgs::wave_div / wave_max): with the length on the device the kernel applies the
            // rule itself, here the host does
            long long grid_th = h->grid_f;
            if (ta.wave_max > 0) grid_th = std::min<long long>(grid_th, ta.wave_max);
            if (!theta_lean && ta.wave_div > 0) grid_th = std::min<long long>(grid_th, std::max<long long>(256, n_theta / ta.wave_div));
            if (!theta_lean) ta.chunk = (int)std::max<long long>(1, std::min<long long>(16, n_theta / (grid_th * 8)));
            const dim3 g((unsigned)std::min<long long>(theta_lean ? n_theta : (n_theta + ta.chunk - 1) / ta.chunk, grid_th));
            if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[0], st));
            launch_theta2(h->fast_t, g, h->lds_f, st, pf, fr, n_theta, k, stp, ctr, kkc, kkl, ta, theta_list);
            if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[1], st));
            kernel_timed[0] = true;
            n_theta_items = n_theta;
            HIP_TRY(h, hipGetLastError());
        }
        return MPC_OK;
    }

    // the dictionary cache of the (x,theta) stage, then the partition behind the theta stage in its three forms: x_first, early_xq, plain
    int first_partition() {
        // ---- (x,theta) stage with the dictionary cache -------------------------------------------------------------
        nxc = dict_nxc(h);
        { int rcs = dict_cache_begin(h, nn, gen_children, st, dc); if (rcs) return rcs; }
        if (h->storing) { int rcs = prep_zero(h->dict_stored[h->dict_cur].p, nn); if (rcs) return rcs; }
        // (behind the theta kernel: everything the main stream and the side streams launch from here on may read dictionary records)
        { int rcj = x1_join(h); if (rcj) return rcj; }
        // One partition after the theta stage: [0] numerically doubtful (status 7), [1] feasible and [2] optimal (decided
        // in theta space; they only need a dictionary for their children), [3] feasibility still open.
        const bool x_first = !early_xq && h->storing && dc.parent_slot && h->kn.x1 > 0 && n >= std::max<long long>(h->kn.x1_min, h->kn.x_first_min) && n <= h->kn.x_first_max &&
                             n <= 0x7fffffffLL && !(flags & MPC_LEVEL_GRAPH);
        if (x_first) {
            { int rcs = partition({{ST_RETRY, 0}, {ST_FEASIBLE, 1}, {ST_OPT_PENDING, 2}, {ST_NEEDX, 3}, {ST_NEEDX_SING, 3}}, cntA, true, dcnt + DC_XFIRST_CLASS); if (rcs) return rcs; }
            hipLaunchKernelGGL(k_publish_words, dim3(1), dim3(64), 0, st, reinterpret_cast<const unsigned int *>(dcnt + DC_XFIRST_CLASS), reinterpret_cast<unsigned int *>(h->tot_dev + 12), PART_CLASSES);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipEventRecord(h->ev_part, st));
            dc.pre1 = part_list(1); dc.pre2 = part_list(2);
            if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[2], st));
            { int rcs = launch_plans(part_list(3), (int)n, n, dcnt + DC_XFIRST_OPEN, dcnt + DC_XFIRST_FEASIBLE, dcnt + DC_XFIRST_OPT); if (rcs) return rcs; }
            if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[3], st));
            kernel_timed[1] = true;
            x_done = true;
            HIP_TRY(h, hipEventSynchronize(h->ev_part));      // the counts that size the region stage (and the doubtful candidates' side stream)
            for (int c = 0; c < PART_CLASSES; ++c) cntA[c] = h->tot_host[12 + c];
        } else if (early_xq) {
            // The thread pass is still rewriting the statuses of ITS candidates (NEEDX -> feasible / infeasible / singular) on the second
            // stream: this partition asks only for the two classes it never touches -- doubtful and optimal candidates of the theta
            // stage --, so that the region stage can start beside it; the open candidates are listed when the pass has ended (below).
            { int rcs = partition({{ST_RETRY, 0}, {ST_OPT_PENDING, 2}}, cntA); if (rcs) return rcs; }
            cntA[3] = (int32_t)std::min<long long>(n, 0x7fffffffLL);     // a bound, for the decisions that follow; the count comes after the join
        } else { int rcs = partition({{ST_RETRY, 0}, {ST_FEASIBLE, 1}, {ST_OPT_PENDING, 2}, {ST_NEEDX, 3}, {ST_NEEDX_SING, 3}}, cntA); if (rcs) return rcs; }
        return MPC_OK;
    }

    // The doubtful candidates are re-solved by the LDS engine, which can refactorise its basis: a few hundred
    // long-running wavefronts.  They run on the side stream while the (x,theta) stage fills the GPU; their results are
    // applied to the status array after the join.
    int doubtful_side_stream() {
        n_early = cntA[0];
        if (n_early > 0) {
            HIP_TRY(h, h->vretry_list.ensure(nn * sizeof(int32_t), st));
            HIP_TRY(h, h->status_tmp.ensure(nn, st));
            if (x_done) {   // (the main stream already carries the (x,theta) stage: the side stream starts behind the partition's event)
                HIP_TRY(h, hipStreamWaitEvent(h->stream2, h->ev_part, 0));
                HIP_TRY(h, hipMemcpyAsync(h->vretry_list.p, part_list(0), (size_t)n_early * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream2));
            } else {
                HIP_TRY(h, hipMemcpyAsync(h->vretry_list.p, part_list(0), (size_t)n_early * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
                HIP_TRY(h, hipEventRecord(h->ev_fork, st));
                HIP_TRY(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
            }
            hipLaunchKernelGGL(k_verdict, dim3((unsigned)std::min<long long>(n_early, h->grid_v)), dim3(64), h->lds_v, h->stream2, h->Pv,
                               h->frontier.as<int32_t>(), (long long)n_early, k, h->status_tmp.as<uint8_t>(), ctr, h->vretry_list.as<int32_t>(), (const int32_t *)nullptr);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipEventRecord(h->ev_join, h->stream2));
        }
        return MPC_OK;
    }

    // The region stage needs the theta stage's verdicts only (no later stage turns a candidate optimal, except the
    // re-solved doubtful ones): it starts now on its own stream and runs under the (x,theta) stage -- a few thousand
    // long wavefronts at two per SIMD whose tail the streaming kernels of the (x,theta) stage fill.
    int overlapped_region_launch() {
        // x_items: what the (x,theta) stage has to do.  Below roverlap_min items there is nothing to hide the region stage
        // under; from roverlap_long items on the stage outlasts the region kernel anyway, which then runs one wavefront per
        // candidate (splitting a candidate over four wavefronts shortens its latency but takes registers from four SIMDs).
        const long long x_items = (long long)cntA[3] + (h->storing ? (long long)cntA[1] + cntA[2] : 0);
        // (the grouped quick test keeps four 128-register wavefronts per SIMD busy through LDS latency: one region wavefront on
        // a CU halves that CU's share of it -- config 3's last level loses 0.1-0.25 ms with the region stage under it)
        lds_q = (size_t)h->dict_stride_d * sizeof(double) + (size_t)h->dict_stride_i * sizeof(int32_t);
        quick_test_on = cntA[3] > 0 && !(flags & MPC_LEVEL_GRAPH) && !h->storing && dc.parent_slot;
        use_grouped = quick_test_on && h->last_level_n > 0 && (long long)cntA[3] >= 10 * h->last_level_n &&
                      cntA[3] >= 4096 && lds_q <= 64 * 1024 && !early_xq;   // (after the thread pass few candidates per parent are left)
        if (!h->kn.no_roverlap && !h->theta_open && cntA[2] > 0 && h->fast_r >= 0 && !(flags & MPC_LEVEL_GRAPH) && x_items >= h->kn.roverlap_min && !use_grouped) {
            // Candidates that turn out optimal later -- re-solved doubtful ones: the n_early of the theta stage, rarely one of
            // the (x,theta) stage -- get spare slots behind the launch's and take the LDS-engine route of the candidates
            // k_region2 gives up on.  The spare slots cover every re-solved candidate of the theta stage plus up to 1,024 of the
            // (x,theta) stage (candidates whose theta stage found no feasible parameter and whose re-solve, in other arithmetic,
            // calls them optimal: none has been seen).  A candidate is never demoted for want of a slot: late candidates beyond
            // the spare slots make the level fail with MPC_ERR_CAPACITY, and the driver repeats the solve with the region stage
            // behind the (x,theta) stage (mpc_set_region_overlap(h, 0)), where every optimal candidate is known at launch.
            const int32_t hold = std::min<int32_t>(std::max(h->kn.test_late, 0), cntA[2] - 1);
            const int32_t n_launch = cntA[2] - hold;
            region_extra = std::max(0, n_early + hold + std::min<int32_t>(cntA[3], 1024) - std::max(h->kn.test_spare, 0));
            rprep.copy_dst = h->opt_list.as<int32_t>(); rprep.copy_src = part_list(2); rprep.copy_n = n_launch; rprep_any = true;
            h->opt_ptr = h->opt_list.as<int32_t>();
            h->n_opt = n_launch;
            int rcs = region2_launch(n_launch, region_extra, h->stream3, x_items >= h->kn.roverlap_long);
            if (rcs) return rcs;
            region_launched = true;
        }
        return MPC_OK;
    }

    // what the (x,theta) stage has to do: the decided candidates that only need a dictionary, and the list of the open ones
    int open_list() {
        if (h->storing) {
            // candidates the theta stage already decided (feasible / optimal) expand too: their children get a
            // dictionary to start from (status untouched).  They ride in front of the open candidates in the same launch.
            dc.pre1 = part_list(1); dc.n_pre1 = cntA[1];
            dc.pre2 = part_list(2); dc.n_pre2 = cntA[2];
        }
        if (early_xq) {
            // the thread pass has ended: what it left open (and what the theta stage left open) is listed now
            HIP_TRY(h, hipStreamWaitEvent(st, h->ev_xjoin, 0));
            int32_t n_left = 0;
            { int rcs = compact(ST_NEEDX, ST_NEEDX_SING, &n_left); if (rcs) return rcs; }
            std::swap(h->xq_list, h->retry_list);     // (xq_list held the pass's input: free again)
            cntA[3] = n_left;
        }
        n_needx = cntA[3];
        needx_list = early_xq ? h->xq_list.as<int32_t>() : part_list(3);
        h->n_needx = n_needx;
        if ((flags & MPC_LEVEL_GRAPH) && n_needx > 0) {
            // connected-graph traversal: only "is the critical region non-empty" is asked; the candidates whose theta stage
            // left feasibility open simply have no region
            hipLaunchKernelGGL(k_close_open, dim3((unsigned)((n_needx + 255) / 256)), dim3(256), 0, st, needx_list, (int)n_needx, stp);
            HIP_TRY(h, hipGetLastError());
            n_needx = 0;
        }
        return MPC_OK;
    }

    int quick_test() {
        if (quick_test_on) {
            // last level: decisions only -- the quick test on three vectors of the parent's dictionary first
            DictCache dq = dc;
            const long long grid_q = (long long)h->n_cu * h->kn.xq_wpc;
            if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[8], st));
            n_xq_items = n_needx;
            // First pass, one THREAD per candidate (k_xq_thread, round 5): whatever the first ratio test of the hinted column
            // decides -- against the generating parent's record, then against the records of the candidate's OTHER parents (the
            // previous level's sets that lack one of its other members).  What stays open is compacted (length on the device) and
            // goes to the wavefront kernel unchanged.  Against the generating parent alone the pass decides 67 % of config 4's
            // last level and gains nothing (the wavefront kernel's time is the other third, candidates that need two to sixteen
            // dependent pivots from THAT vertex: level 5 2.36 ms with, 2.35 without); from another parent's vertex almost all
            // of those are one ratio test away too: 99.76 % decided, level 5 2.35 -> 1.75 ms; config 3 93 %, 4.75 -> 3.43 ms.
            const int32_t *xq_list = needx_list;
            int32_t xq_n = n_needx;
            bool xqt_lean = false;
            if (h->kn.xq_thread != 0 && n_needx >= h->kn.xqt_min && !early_xq) {
                const unsigned gt = (unsigned)std::min<long long>(((long long)n_needx + 63) / 64, (long long)h->n_cu * h->kn.xqt_wpc);
                if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[10], st));
                XqAlt alt{};
                if ((h->kn.xq_thread >= 2 || h->kn.xq_thread < 0) && h->have_prev_dict) alt = other_parents(h->kn.xq_thread < 0 ? MPC_MAX_NC : h->kn.xq_thread - 1);
                hipLaunchKernelGGL(k_xq_thread, dim3(gt), dim3(64), 0, st, pf, fr, k, needx_list, n_needx, stp, ctr, dq, nxc, alt, XqPlan{});
                if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[11], st));
                HIP_TRY(h, hipGetLastError());
                xq_thread_timed = true;
                if (!use_grouped) { int rcs = compact(ST_NEEDX, ST_NEEDX_SING, nullptr, dcnt + DC_OPEN_XQT); if (rcs) return rcs; xqt_lean = true; }   // (the grouped form sizes its group scan on the host)
                else { int32_t n_left = 0; int rcs = compact(ST_NEEDX, ST_NEEDX_SING, &n_left); if (rcs) return rcs; xq_n = n_left; }
                HIP_TRY(h, h->xq_list.ensure(nn * sizeof(int32_t), st));
                std::swap(h->xq_list, h->retry_list);   // compact() filled retry_list; keep it as the wavefront kernel's list
                xq_list = h->xq_list.as<int32_t>();
            }
            dq.chunk = (int)std::max<long long>(1, std::min<long long>(16, xq_n / (grid_q * 4)));
            if (xqt_lean) { dq.n_list_dev = dcnt + DC_OPEN_XQT; dq.chunk = 0; dq.skip_below = (h->fast_x & 1) ? 0 : h->kn.xq_skip_below; }   // length and chunk rule on the device; a short list is left to k_x2
            const dim3 gg((unsigned)std::max<long long>(1, std::min<long long>(xqt_lean ? (long long)xq_n : ((long long)xq_n + dq.chunk - 1) / dq.chunk, grid_q)));
            // Grouped by parent when a parent has many open children (config 3: 12.6 per parent, -0.5 ms; config 4: 7.1 per
            // parent, where the per-candidate reads of k_xq are cheaper than one 16 KB copy per parent, +0.45 ms): threshold 10.
            if (use_grouped && xq_n > 0) {
                // grouped by parent: the record is staged in LDS once per parent (k_xq_grouped)
                HIP_TRY(h, h->xq_groups.ensure((size_t)xq_n * sizeof(int32_t), st));
                const int nbq = (xq_n + 255) / 256;
                hipLaunchKernelGGL(k_group_flags, dim3(nbq), dim3(256), 0, st, xq_list, xq_n, dq.parent_slot, h->flag.as<int32_t>());
                { int rcs = launch_scan(h, h->flag.as<int32_t>(), h->pos.as<int32_t>(), xq_n, h->scratch.as<int32_t>()); if (rcs) return rcs; }
                hipLaunchKernelGGL(k_scatter_index, dim3(nbq), dim3(256), 0, st, h->flag.as<int32_t>(), h->pos.as<int32_t>(), (long long)xq_n, h->xq_groups.as<int32_t>());
                const int per_cu = std::max(1, std::min(h->kn.xqg_per_cu, (int)((160 * 1024) / (lds_q + 64))));
                const dim3 gq((unsigned)std::min<long long>(xq_n, (long long)h->n_cu * per_cu)), bq(256);
                if (lds_q > 48 * 1024) {
                    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_xq_grouped<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_q));
                    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_xq_grouped<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_q));
                }
                if (h->fast_x & 1) hipLaunchKernelGGL((k_xq_grouped<2>), gq, bq, lds_q, st, pf, fr, k, xq_list, xq_n, stp, ctr, dq, nxc, h->xq_groups.as<int32_t>(), h->scratch.as<int32_t>());
                else hipLaunchKernelGGL((k_xq_grouped<1>), gq, bq, lds_q, st, pf, fr, k, xq_list, xq_n, stp, ctr, dq, nxc, h->xq_groups.as<int32_t>(), h->scratch.as<int32_t>());
            } else if (xq_n == 0) { /* the first pass decided everything (host-known length) */ }
            else if (!xqt_lean && !(h->fast_x & 1) && xq_n < h->kn.xq_skip_below) { /* a short list (host-known length) is left to k_x2: k_xq's comment */ }
            else launch_xq(h->fast_x, gg, st, pf, fr, k, xq_list, xq_n, stp, ctr, dq, nxc);
            if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[9], st));
            kernel_timed[4] = true;
            HIP_TRY(h, hipGetLastError());
            { int rcs = compact(ST_NEEDX, ST_NEEDX_SING, nullptr, dcnt + DC_OPEN_QT); if (rcs) return rcs; }
            xq_lean = true;   // n_needx stays the bound (everything the quick test was given)
            needx_list = h->retry_list.as<int32_t>();
        }
        return MPC_OK;
    }

    int x_stage() {
        if (x_done) n_x_items = n_needx + dc.n_pre1 + dc.n_pre2;      // (queued behind the partition, above)
        else if (n_needx + dc.n_pre1 + dc.n_pre2 > 0) {   // feasibility for the candidates left open (+ dictionary-only items)
            if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[2], st));
            int rcs = MPC_OK;
            const long long n_dict = (long long)n_needx + dc.n_pre1 + dc.n_pre2;
            if (h->storing && dc.parent_slot && h->kn.x1 > 0 && !xq_lean && n_dict >= h->kn.x1_min) {
                rcs = launch_plans(needx_list, n_needx, n_dict, nullptr, nullptr, nullptr);
            } else rcs = launch_x(needx_list, n_needx, dc);
            if (rcs) return rcs;
            if (h->timing) HIP_TRY(h, hipEventRecord(h->kev[3], st));
            kernel_timed[1] = true;
            n_x_items = n_needx + dc.n_pre1 + dc.n_pre2;
        }
        // A storing level without (x,theta) items has not flushed `prep` (launch_x does): the clear of dict_stored[dict_cur] queued in it
        // must still run before k_children_write reads that array (stale "stored" bytes of two levels ago would send a child
        // to another candidate's dictionary).
        { int rcs = prep_flush(); if (rcs) return rcs; }
        return MPC_OK;
    }

    // the join of the re-solved doubtful candidates of the theta stage, and -- behind an overlapped region launch -- the speculative end of the level
    int second_partition_and_tail() {
        // doubtful candidates of the (x,theta) stage (rare) take the same route on the main stream
        if (n_early > 0) {
            // the early retries still carry status 7: mark them so that this compaction does not pick them up again
            HIP_TRY(h, hipStreamWaitEvent(st, h->ev_join, 0));
            hipLaunchKernelGGL(k_apply_status, dim3((unsigned)((n_early + 255) / 256)), dim3(256), 0, st, h->vretry_list.as<int32_t>(), (int)n_early,
                               h->status_tmp.as<uint8_t>(), stp);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipMemsetAsync(&ctr->work_retry, 0, sizeof(unsigned int), st));
        }
        // second partition: [0] doubtful candidates of the (x,theta) stage, [2] the optimal candidates for the region stage
        if (region_launched) HIP_TRY(h, hipStreamWaitEvent(st, h->ev_rjoin, 0));   // the region kernel rewrites statuses
        if (region_launched) {
            // The overlapped region stage has finished (the stream waits for it above), so in the usual case nothing is left to do but
            // the end of the level: no doubtful candidate of the (x,theta) stage, no late optimal one, none that k_region2 gave up on.
            // The three counts that say so used to cost three host round trips (this partition, the n_rretry read-back, the final one:
            // 45-70 us of idle device per large level, tools/timeline.sh); now the end of the level is queued right behind the
            // partition, ONE synchronisation reads everything, and only when a count is not zero the classic sequence below runs and
            // the end of the level is repeated (its two accumulating counters are cleared; everything else it wrote is overwritten).
            { int rcs = partition({{ST_RETRY, 0}, {ST_OPT_PENDING, 2}}, cntB, true); if (rcs) return rcs; }
            hipLaunchKernelGGL(k_publish_words, dim3(1), dim3(64), 0, st, &ctr->n_rretry, reinterpret_cast<unsigned int *>(h->tot_dev + 8), 1);
            if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[1], st));
            if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[2], st));
            { int rcs = queue_tail(); if (rcs) return rcs; }
            HIP_TRY(h, hipStreamSynchronize(st));
            for (int c = 0; c < PART_CLASSES; ++c) cntB[c] = h->tot_host[12 + c];
            have_cntB = true;
            if (cntB[0] == 0 && cntB[2] == 0 && h->tot_host[8] == 0) tail_done = true;
            else {
                HIP_TRY(h, hipMemsetAsync(&ctr->n_pruned_new, 0, sizeof(unsigned int), st));
                HIP_TRY(h, hipMemsetAsync(ctr->status, 0, sizeof(ctr->status), st));
                h->n_children = 0;
            }
        }
        return MPC_OK;
    }

    // the classic sequence behind the (x,theta) stage: its doubtful candidates re-solved, late optimal candidates into the spare slots
    int retry_and_late() {
        int32_t n_retry = 0;
        { int rcs = recession(); if (rcs) return rcs; }
        if (!have_cntB) { int rcs = partition({{ST_RETRY, 0}, {ST_OPT_PENDING, 2}}, cntB); if (rcs) return rcs; }
        n_retry = cntB[0];
        if (n_retry > 0 && !region_launched && !h->kn.no_roverlap && !h->theta_open && cntB[2] > 0 && h->fast_r >= 0 && !(flags & MPC_LEVEL_GRAPH)) {
            // the region stage was not started under the (x,theta) stage (grouped quick test, short stage): it runs beside the
            // re-solve of the doubtful candidates instead -- two small, latency-bound kernels; what the re-solve finds optimal
            // takes the spare slots (config 3's last level: 235 re-solved candidates, 0.4 ms)
            region_extra = n_retry;
            rprep.copy_dst = h->opt_list.as<int32_t>(); rprep.copy_src = part_list(2); rprep.copy_n = cntB[2]; rprep_any = true;   // (on the region kernel's stream)
            h->opt_ptr = h->opt_list.as<int32_t>();
            h->n_opt = cntB[2];
            int rcs = region2_launch(cntB[2], region_extra, h->stream3, false);
            if (rcs) return rcs;
            region_launched = true;
        }
        if (n_retry > 0) {
            hipLaunchKernelGGL(k_verdict, dim3((unsigned)std::min<long long>(n_retry, h->grid_v)), dim3(64), h->lds_v, st, h->Pv,
                               h->frontier.as<int32_t>(), (long long)n_retry, k, h->status.as<uint8_t>(), ctr, part_list(0), (const int32_t *)nullptr);
            HIP_TRY(h, hipGetLastError());
            if (region_launched) HIP_TRY(h, hipStreamWaitEvent(st, h->ev_rjoin, 0));
            { int rcs = recession(); if (rcs) return rcs; }
            { int rcs = partition({{ST_OPT_PENDING, 2}}, cntB); if (rcs) return rcs; }   // they may have turned out optimal
        }
        if (region_launched) {
            n_late = cntB[2];
            const int32_t *late = part_list(2);
            if (n_late > region_extra)
                return fail(h, MPC_ERR_CAPACITY, "late optimal candidates (" + std::to_string(n_late) + ") exceed the spare region slots (" + std::to_string(region_extra) +
                                                 ") of the overlapped region stage: repeat the solve after mpc_set_region_overlap(h, 0)");
            if (n_late > 0) {
                const int32_t n_a = (int32_t)h->n_opt;
                HIP_TRY(h, hipMemcpyAsync(h->opt_list.as<int32_t>() + n_a, late, (size_t)n_late * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
                hipLaunchKernelGGL(k_init_slots, dim3((unsigned)((n_late + 255) / 256)), dim3(256), 0, st, region_out_hi, h->fi, n_a, n_late, ST_RETRY, late);
                HIP_TRY(h, hipGetLastError());
                h->n_opt = n_a + n_late;
            }
            n_opt_fast = (int32_t)h->n_opt;
        } else {
            n_opt_fast = cntB[2];
            h->opt_ptr = part_list(2);   // stays valid until the next level's partition (the region fetch reads it before that)
        }
        return MPC_OK;
    }

    // the verdict stage without the register engine (no pre-crashed dictionary, or MPC_FORCE_V1): k_verdict for every candidate
    int plain_verdict() {
        hipLaunchKernelGGL(k_verdict, dim3((unsigned)std::min<long long>(n, h->grid_v)), dim3(64), h->lds_v, st, h->Pv,
                           h->frontier.as<int32_t>(), n, k, h->status.as<uint8_t>(), ctr, (const int32_t *)nullptr, (const int32_t *)nullptr);
        HIP_TRY(h, hipGetLastError());
        { int rcs = recession(); if (rcs) return rcs; }
        return MPC_OK;
    }

    int region_stage() {
        if (!tail_done) if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[1], st));
        // optimal candidates -> region kernel
        int32_t n_opt = n_opt_fast;
        if (n_opt < 0) {
            h->opt_ptr = h->opt_list.as<int32_t>();
            hipLaunchKernelGGL(k_flag_status, dim3(blocks256), dim3(256), 0, st, h->status.as<uint8_t>(), n, ST_OPT_PENDING, ST_OPT_PENDING, h->flag.as<int32_t>());
            { int rcs = launch_scan(h, h->flag.as<int32_t>(), h->pos.as<int32_t>(), n, total); if (rcs) return rcs; }
            hipLaunchKernelGGL(k_scatter_index, dim3(blocks256), dim3(256), 0, st, h->flag.as<int32_t>(), h->pos.as<int32_t>(), n, h->opt_list.as<int32_t>());
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipStreamSynchronize(st));
            n_opt = h->tot_host[0];
        }
        h->n_opt = n_opt;
        if (tail_done) { /* the overlapped region stage left nothing to do: see the speculative end of the level above */ }
        else if (n_opt > 0 && h->fast && h->fast_r >= 0 && !h->kn.force_v1) {
            if (!region_launched) { int rcs = region2_launch(n_opt, 0, st, false); if (rcs) return rcs; }
            // candidates k_region2 gave up on (counted by the kernel; normally none): the LDS-engine kernel, fixed-stride records
            hipLaunchKernelGGL(k_publish_words, dim3(1), dim3(64), 0, st, &ctr->n_rretry, reinterpret_cast<unsigned int *>(h->tot_dev + 8), 1);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipStreamSynchronize(st));
            const unsigned int n_rr_dev = (unsigned int)h->tot_host[8];
            int32_t n_rr = 0;
            if (n_rr_dev > 0) { int rcs = compact(ST_RRETRY, ST_RRETRY, &n_rr); if (rcs) return rcs; }
            if (n_late > 0) {   // the late optimal candidates follow, in the order of their slots
                HIP_TRY(h, h->retry_list.ensure(nn * sizeof(int32_t), st));
                HIP_TRY(h, hipMemcpyAsync(h->retry_list.as<int32_t>() + n_rr, h->opt_list.as<int32_t>() + (n_opt - n_late), (size_t)n_late * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
                n_rr += n_late;
            }
            h->n_rretry = n_rr;
            if (n_rr > 0) {   // numerically doubtful regions: the LDS-engine kernel, fixed-stride records
                int rcs = launch_region_v1(h, h->retry_list.as<int32_t>(), n_rr, k, ctr);
                if (rcs) return rcs;
            }
        } else if (n_opt > 0) {
            int rcs = launch_region_v1(h, h->opt_ptr, n_opt, k, ctr);
            if (rcs) return rcs;
        }
        return MPC_OK;
    }

    int tail() {
        if (!tail_done) {
            if (h->timing) HIP_TRY(h, hipEventRecord(h->ev[2], st));
            // pruned masks of this level + children, histogram, counters
            { int rcs = queue_tail(); if (rcs) return rcs; }
            HIP_TRY(h, hipStreamSynchronize(st));
        }
        return MPC_OK;
    }

    // behind the level's closing synchronisation: the published counters and list lengths, the event times, the debug prints
    int read_back() {
        if (prep_any || rprep_any) return fail(h, MPC_ERR_STATE, "level_run: a queued preparation (clear / copy) was never issued");
        h->r3_dirty = false;   // the main stream waited for ev_rjoin before the second partition
        std::memcpy(&host_ctr, h->tot_host + 16, sizeof(LevelCounters));
        const int32_t *cnt_host = h->cnt_host();
        if (children_lean) h->n_children = cnt_host[DC_CHILDREN];
        if (theta_lean) n_theta_items = cnt_host[DC_THETA];
        if (xq_lean) n_x_items = (long long)cnt_host[DC_OPEN_QT] + (n_x_items - n_xq_items);   // what the quick test left + the dictionary-only items
        if (h->timing) HIP_TRY(h, hipEventElapsedTime(&ms[0], h->ev[0], h->ev[1]));
        if (h->timing) HIP_TRY(h, hipEventElapsedTime(&ms[1], h->ev[1], h->ev[2]));
        if (h->timing) HIP_TRY(h, hipEventElapsedTime(&ms[2], h->ev[2], h->ev[3]));
        for (int i = 0; i < 5; ++i) if (kernel_timed[i] && h->timing) HIP_TRY(h, hipEventElapsedTime(&kms[i], h->kev[2 * i], h->kev[2 * i + 1]));
        if ((xq_thread_timed) && h->timing) { HIP_TRY(h, hipEventElapsedTime(&h->ms_xq_thread, h->kev[10], h->kev[11])); h->n_xq_thread = host_ctr.xq_thread; }
        h->ms_x1 = 0;
        if ((x1_ran) && h->timing) HIP_TRY(h, hipEventElapsedTime(&h->ms_x1, h->kev[12], h->kev[13]));
        h->n_x1 = x1_ran ? (long long)cnt_host[DC_X1] : 0;   // dictionaries k_x1 wrote
        if (h->kn.debug_cycles && x1_ran) { const int32_t *ch = cnt_host; std::fprintf(stderr, "[mpc] k=%d one-step plans: %d streamed by k_x1, %d + %d + %d left to k_x2 (plan pass %.3f ms)\n", k, ch[DC_X1], ch[DC_X1_REST], ch[DC_X1_REST + 1], ch[DC_X1_REST + 2], h->ms_xq_thread); }
        if (xq_early_ran) { n_xq_items += host_ctr.xq_thread; h->n_needx += host_ctr.xq_thread; }   // what the pass beside the theta stage decided never reached the partition's count
        if (kernel_timed[2] && host_ctr.r2_t1 > ~host_ctr.r2_not_t0 && h->wall_khz > 0)   // k_region2 times itself (see the kernel)
            kms[2] = (float)((double)(host_ctr.r2_t1 - ~host_ctr.r2_not_t0) / (double)h->wall_khz);
        if (h->kn.debug_cycles)
            std::fprintf(stderr, "[mpc] k=%d n=%lld cycles/cand: kkt %.0f theta %.0f (rows %.0f, stage2 %.0f) x %.0f region %.0f; pivots %.2f; box screen %.3f / %.3f; x quick %.3f; retries theta %u of %llu\n", k, n,
                         host_ctr.cycles[0] / (double)n, host_ctr.cycles[1] / (double)n, host_ctr.cycles[4] / (double)n, host_ctr.cycles[5] / (double)n,
                         host_ctr.cycles[2] / (double)n, host_ctr.cycles[3] / (double)n, host_ctr.pivots / (double)n, host_ctr.cycles[6] / (double)n, host_ctr.cycles[7] / (double)n, host_ctr.xtheta_lps / (double)n, host_ctr.n_retry_theta, (unsigned long long)host_ctr.xtheta_fallbacks);
        if (h->kn.debug_cycles && h->n_opt > 0)
            std::fprintf(stderr, "[mpc] k=%d region2 per optimal candidate (%lld): rows %.0f chebyshev %.0f facets %.0f total %.0f cycles; refactors %.2f facet pivots %.1f box-screened rows %.1f\n", k,
                         h->n_opt, host_ctr.rcycles[0] / (double)h->n_opt, host_ctr.rcycles[1] / (double)h->n_opt, host_ctr.rcycles[2] / (double)h->n_opt,
                         host_ctr.rcycles[3] / (double)h->n_opt, host_ctr.rcycles[4] / (double)h->n_opt, host_ctr.rcycles[5] / (double)h->n_opt, host_ctr.r_box / (double)h->n_opt);
        h->n_pruned_new = host_ctr.n_pruned_new;
        h->n_erows = host_ctr.e_rows;
        h->n_regions = (long long)host_ctr.status[ST_REGION];
        return MPC_OK;
    }

    void fill_stats(mpc_level_stats *stats) const {
        level_stats_common(h, host_ctr, stats);
        stats->n_xtheta_lp = (h->fast && !h->kn.force_v1) ? h->n_needx : (int64_t)host_ctr.xtheta_lps;
        stats->n_region_retry = h->n_rretry;
        stats->ms_theta = kms[0]; stats->ms_x = kms[1]; stats->ms_region2 = kms[2];
        stats->region_side_stream = h->region_side_stream ? 1.0f : 0.0f;
        stats->n_x_items = n_x_items;
        stats->n_theta_items = n_theta_items;
        stats->ms_kkt = kms[3]; stats->ms_xq = kms[4];
        stats->n_xq_items = n_xq_items;
        stats->n_xq_thread = h->n_xq_thread; stats->ms_xq_thread = h->ms_xq_thread; stats->xq_thread_beside_theta = xq_early_ran ? 1.0f : 0.0f;
        stats->n_x1 = h->n_x1; stats->ms_x1 = h->ms_x1; stats->ms_x_plan = x1_ran ? h->ms_xq_thread : 0.0f;
        stats->dict_read_bytes = (h->fast && h->have_prev_dict && h->have_parent_slot) ? dict_record_bytes(h) : 0;
        stats->dict_write_bytes = (h->fast && h->storing) ? dict_record_bytes(h) : 0;
        stats->ms_verdict = ms[0]; stats->ms_region = ms[1]; stats->ms_children = ms[2]; stats->ms_total = ms[0] + ms[1] + ms[2];
    }
};

}  // namespace
