// level_fetch.hpp -- a level's region records off the device: sizes, the slot / compact / fixed fetches, the shared copy launch of a batch
// and the copy launch of the solve loop.  Host only; included by mpcombi_hip.hip behind mpc_handle and the engine's helpers it calls
// (fail, HIP_TRY, host_pool_take, pooled_event, debug_many, record_shape): the translation unit stays one.  The layout of both record forms
// and the conversions between them are records.hpp's; nothing here spells an offset.
//
//   level_record_sizes       fd, fi, slots and the row bound of a level: from the handle's state or from the level's statistics
//   SlotFetch                one slot fetch (mpc_level_regions_slots*, mpc_level_stream_fixup, the solve loop) as stages:
//     check()                  state and capacity; nothing to fetch
//     stage_fixed()            recd, reci, opt list, status -> st_* staging (only with records in fixed form); stage_rlist(): retry_list
//     copy_slots_heads_first() every record in slot form on the device: head_i, event, head_d, rows; waits for the event or for nothing
//     copy_slots()             the ordinary path: head_d, head_i, rows into the caller's arrays (not in_place)
//     debug_reasons()          MPC_DEBUG_CYCLES: region retries by reason
//     fill_fixed()             fixed_to_slot for every slot whose record came in fixed form
//   mpc_level_regions_compact  the same stages into staging, then regions only, frontier order, rows rebased
//   mpc_level_regions          compact, then slot_to_fixed
//   mpc_level_batch_fetch      k_rretry_merge + one k_fetch_many for the members of a batch; fetch_many_wait / mpc_fetch_wait
//   solve_fetch_slots          k_fetch_slots into fresh page-locked blocks of a level of the solve loop
#pragma once

struct RecordSizes { int fd, fi; long long n_slots, rows_cap; };
static RecordSizes record_sizes(const RecordShape &sh, bool pooled, long long n_opt, long long n_erows, long long n_rretry, long long n_regions) {
    return {sh.fd(), sh.fi(), n_opt, record_rows_bound(sh, pooled, n_erows, n_rretry, n_regions)};
}
// of the level the handle has just run
static RecordSizes level_record_sizes(const mpc_handle *h) { return record_sizes(record_shape(h), h->used_region2, h->n_opt, h->n_erows, h->n_rretry, h->n_regions); }
// of a level known by its statistics alone (pooled rows are counted, so there are some); no regions: nothing to fetch
static RecordSizes level_record_sizes(const mpc_handle *h, const mpc_level_stats &st) {
    const RecordShape sh = record_shape(h, st.k);
    if (st.n_regions <= 0) return {sh.fd(), sh.fi(), 0, 0};
    return record_sizes(sh, st.n_region_rows != 0, st.n_opt, st.n_region_rows, st.n_region_retry, st.n_regions);
}

int mpc_compact_strides(const mpc_handle *h, int64_t *fd, int64_t *fi, int64_t *max_rows) {
    if (!h) return MPC_ERR_INVALID;
    const RecordSizes z = level_record_sizes(h);
    if (fd) *fd = z.fd;
    if (fi) *fi = z.fi;
    if (max_rows) *max_rows = z.rows_cap;
    return MPC_OK;
}

int64_t mpc_level_slots(const mpc_handle *h) { return h ? h->n_opt : 0; }

// complete: everything has arrived on return.  heads_first / queued_only: where every record is in slot form on the device the call returns
// when the integer heads have arrived / without waiting at all, the rest in flight on the handle's stream (mpc_sync completes it); otherwise
// as complete.  in_place: the region kernel streamed the records into the caller's arrays; only the slots of candidates re-solved into fixed
// records are filled.
enum class FetchMode { complete, heads_first, queued_only, in_place };

struct SlotFetch {
    mpc_handle *h;
    double *head_d; int32_t *head_i; double *erows;   // the caller's arrays
    RecordShape sh{};
    bool merged = false;                 // k_rretry_merge has written the re-solved candidates' records into their slots
    long long pool_rows = 0, n_fixed = 0;   // rows of epool in use; records in fixed form (recd / reci)

    void derive() {
        sh = record_shape(h);
        merged = h->used_region2 && h->rretry_rows >= 0;
        pool_rows = merged ? h->rretry_rows : h->n_erows;
        n_fixed = h->used_region2 ? (merged ? 0 : h->n_rretry) : h->n_opt;
    }
    bool all_slots_on_device() const { return h->used_region2 && n_fixed == 0; }

    // *empty: the level has no region, nothing is fetched
    int check(FetchMode mode, int64_t cap_slots, int64_t cap_rows, int64_t *n_slots, int64_t *n_rows, bool *empty) {
        *empty = true;
        if (!h->level_done) return fail(h, MPC_ERR_STATE, "mpc_level_run has not been called for this frontier");
        if (h->so.active && mode != FetchMode::in_place) return fail(h, MPC_ERR_STATE, "the records of this level were streamed to the host (mpc_level_stream_info)");
        if (n_slots) *n_slots = 0;
        if (n_rows) *n_rows = 0;
        if (h->n_regions == 0 || h->n_opt == 0) return MPC_OK;
        if (cap_slots < h->n_opt) return fail(h, MPC_ERR_CAPACITY, "slot buffers too small (mpc_level_slots)");
        if (!head_d || !head_i || !erows) return MPC_ERR_INVALID;
        HIP_TRY(h, hipSetDevice(h->device));
        derive();
        if (cap_rows < (merged ? pool_rows : level_record_sizes(h).rows_cap)) return fail(h, MPC_ERR_CAPACITY, "row buffer too small (see mpc_compact_strides max_rows)");
        *empty = false;
        return MPC_OK;
    }
    int stage_records() {
        if (n_fixed <= 0) return MPC_OK;
        const size_t bd = (size_t)n_fixed * h->rec_d * sizeof(double), bi = (size_t)n_fixed * h->rec_i * sizeof(int32_t);
        HIP_TRY(h, h->st_fxd.ensure(bd));
        HIP_TRY(h, h->st_fxi.ensure(bi));
        HIP_TRY(h, hipMemcpyAsync(h->st_fxd.p, h->recd.p, bd, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->st_fxi.p, h->reci.p, bi, hipMemcpyDeviceToHost, h->stream));
        return MPC_OK;
    }
    int stage_lists() {
        HIP_TRY(h, h->st_list.ensure((size_t)h->n_opt * sizeof(int32_t)));
        HIP_TRY(h, h->st_status.ensure((size_t)h->n));
        HIP_TRY(h, hipMemcpyAsync(h->st_list.p, h->opt_ptr, (size_t)h->n_opt * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->st_status.p, h->status.p, (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
        return MPC_OK;
    }
    int stage_rlist() {
        if (!h->used_region2 || h->n_rretry <= 0 || merged) return MPC_OK;
        HIP_TRY(h, h->st_rlist.ensure((size_t)h->n_rretry * sizeof(int32_t)));
        HIP_TRY(h, hipMemcpyAsync(h->st_rlist.p, h->retry_list.p, (size_t)h->n_rretry * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        return MPC_OK;
    }
    // what fill_fixed reads, queued on the handle's stream (the retry list follows the slot copies: stage_rlist)
    int stage_fixed() {
        if (n_fixed <= 0) return MPC_OK;
        // every staging block first (a block that grows is taken from the page-locked pool before any copy is queued), then the four copies
        HIP_TRY(h, h->st_fxd.ensure((size_t)n_fixed * h->rec_d * sizeof(double)));
        HIP_TRY(h, h->st_fxi.ensure((size_t)n_fixed * h->rec_i * sizeof(int32_t)));
        HIP_TRY(h, h->st_list.ensure((size_t)h->n_opt * sizeof(int32_t)));
        HIP_TRY(h, h->st_status.ensure((size_t)h->n));
        if (int rc = stage_records()) return rc;
        return stage_lists();
    }
    // the three slot arrays device -> dst_*, in the given order of the two heads
    int queue_slots(double *dst_d, int32_t *dst_i, double *dst_rows, bool ints_first, hipEvent_t after_ints) {
        const size_t bd = (size_t)h->n_opt * sh.fd() * sizeof(double), bi = (size_t)h->n_opt * sh.fi() * sizeof(int32_t);
        if (!ints_first) HIP_TRY(h, hipMemcpyAsync(dst_d, h->headd.p, bd, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(dst_i, h->headi.p, bi, hipMemcpyDeviceToHost, h->stream));
        if (after_ints) HIP_TRY(h, hipEventRecord(after_ints, h->stream));
        if (ints_first) HIP_TRY(h, hipMemcpyAsync(dst_d, h->headd.p, bd, hipMemcpyDeviceToHost, h->stream));
        if (pool_rows > 0) HIP_TRY(h, hipMemcpyAsync(dst_rows, h->epool.p, (size_t)pool_rows * sh.row_len() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        return MPC_OK;
    }
    // the small integer heads first, then the two large arrays
    int copy_slots_heads_first(bool wait_for_heads) {
        if (int rc = queue_slots(head_d, head_i, erows, true, h->ev_hi)) return rc;
        if (wait_for_heads) HIP_TRY(h, hipEventSynchronize(h->ev_hi));
        return MPC_OK;
    }
    int copy_slots() { return queue_slots(head_d, head_i, erows, false, nullptr); }
    void debug_reasons() const {
        long long hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (long long w = 0; w < h->n_opt; ++w) { const int32_t *oi = head_i + (size_t)w * sh.fi(); if (oi[SW_STATUS] == ST_RETRY) hist[oi[SW_REASON] & 7]++; }
        std::fprintf(stderr, "[mpc] k=%d region retries by reason: chebyshev %lld, r->0 %lld, refactor-after-chebyshev %lld, row lost %lld, >8 refactors %lld, refactor failed %lld\n",
                     sh.k, hist[1], hist[2], hist[3], hist[4], hist[5], hist[6]);
    }
    // the staged fixed record of slot w (candidate cand), nullptr: none.  Without k_region2 every slot has one, in slot order; with it the
    // slots marked ST_RETRY have theirs in the order of the retry list (*rpos: the walk through it).
    bool fixed_of(long long w, int cand, bool retry_slot, long long *rpos, const double **rd, const int32_t **ri) const {
        long long src = -1;
        if (!h->used_region2) src = w;
        else if (retry_slot) {
            const int32_t *rlist = h->st_rlist.as<int32_t>();
            while (*rpos < h->n_rretry && rlist[*rpos] != cand) ++*rpos;
            if (*rpos < h->n_rretry) src = *rpos;
        } else return false;
        *rd = src < 0 ? nullptr : h->st_fxd.as<double>() + (size_t)src * h->rec_d;
        *ri = src < 0 ? nullptr : h->st_fxi.as<int32_t>() + (size_t)src * h->rec_i;
        return true;
    }
    // the candidates solved by the LDS-engine kernel come as fixed-stride records: written into their slots here.  Returns the rows in use.
    long long fill_fixed() {
        long long wrow = h->used_region2 ? pool_rows : 0, rpos = 0;
        if (n_fixed <= 0) return wrow;
        const int32_t *list = h->st_list.as<int32_t>();
        const uint8_t *st = h->st_status.as<uint8_t>();
        for (long long w = 0; w < h->n_opt; ++w) {
            const int cand = list[w];
            int32_t *oi = head_i + (size_t)w * sh.fi();
            const double *rd = nullptr; const int32_t *ri = nullptr;
            if (!fixed_of(w, cand, oi[SW_STATUS] == ST_RETRY, &rpos, &rd, &ri)) continue;
            wrow += fixed_to_slot(sh, rd, ri, st[cand], cand, wrow, head_d + (size_t)w * sh.fd(), oi, erows);
        }
        return wrow;
    }
};

static int level_regions_slots_impl(mpc_handle *h, double *head_d, int32_t *head_i, int64_t cap_slots, double *erows, int64_t cap_rows,
                                    int64_t *n_slots, int64_t *n_rows, FetchMode mode) {
    if (!h) return MPC_ERR_INVALID;
    SlotFetch f{h, head_d, head_i, erows};
    bool empty = false;
    if (int rc = f.check(mode, cap_slots, cap_rows, n_slots, n_rows, &empty)) return rc;
    if (empty) return MPC_OK;
    if (int rc = f.stage_fixed()) return rc;
    long long rows = f.pool_rows;
    if (f.all_slots_on_device() && (mode == FetchMode::heads_first || mode == FetchMode::queued_only)) {
        if (int rc = f.copy_slots_heads_first(mode == FetchMode::heads_first)) return rc;
    } else {
        if (h->used_region2 && mode != FetchMode::in_place) if (int rc = f.copy_slots()) return rc;
        if (int rc = f.stage_rlist()) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (h->kn.debug_cycles && h->used_region2) f.debug_reasons();
        rows = f.fill_fixed();
    }
    if (n_slots) *n_slots = h->n_opt;
    if (n_rows) *n_rows = rows;
    return MPC_OK;
}

int mpc_level_regions_slots(mpc_handle *h, double *head_d, int32_t *head_i, int64_t cap_slots, double *erows, int64_t cap_rows,
                            int64_t *n_slots, int64_t *n_rows) {
    return level_regions_slots_impl(h, head_d, head_i, cap_slots, erows, cap_rows, n_slots, n_rows, FetchMode::complete);
}
int mpc_level_regions_slots_async(mpc_handle *h, double *head_d, int32_t *head_i, int64_t cap_slots, double *erows, int64_t cap_rows,
                                  int64_t *n_slots, int64_t *n_rows) {
    return level_regions_slots_impl(h, head_d, head_i, cap_slots, erows, cap_rows, n_slots, n_rows, FetchMode::heads_first);
}
int mpc_level_regions_slots_nowait(mpc_handle *h, double *head_d, int32_t *head_i, int64_t cap_slots, double *erows, int64_t cap_rows,
                                   int64_t *n_slots, int64_t *n_rows) {
    return level_regions_slots_impl(h, head_d, head_i, cap_slots, erows, cap_rows, n_slots, n_rows, FetchMode::queued_only);
}
int mpc_level_stream_fixup(mpc_handle *h, double *head_d, int32_t *head_i, double *erows, int64_t *n_rows) {
    if (!h || !head_d || !head_i || !erows) return MPC_ERR_INVALID;
    if (!h->so.active) return fail(h, MPC_ERR_STATE, "mpc_level_stream_fixup: this level was not streamed");
    { std::lock_guard<std::mutex> lk(h->wm); if (h->w_busy) return fail(h, MPC_ERR_STATE, "the level is still running"); }
    int64_t ns = 0;
    return level_regions_slots_impl(h, head_d, head_i, h->so.n_slots, erows, h->so.cap_rows, &ns, n_rows, FetchMode::in_place);
}

// Regions of the level in compact form, frontier order, written straight into the caller's arrays: only the slots that are regions,
// their rows rebased to the order of the output.
int mpc_level_regions_compact(mpc_handle *h, double *head_d, int32_t *head_i, int64_t cap_regions, double *erows, int64_t cap_rows,
                              int64_t *n_regions, int64_t *n_rows) {
    if (!h) return MPC_ERR_INVALID;
    if (!h->level_done) return fail(h, MPC_ERR_STATE, "mpc_level_run has not been called for this frontier");
    if (n_regions) *n_regions = h->n_regions;
    if (n_rows) *n_rows = 0;
    if (h->so.active) return fail(h, MPC_ERR_STATE, "the records of this level were streamed to the host (mpc_level_stream_info)");
    if (cap_regions < h->n_regions) return fail(h, MPC_ERR_CAPACITY, "region buffers too small");
    if (h->n_regions == 0 || h->n_opt == 0) return MPC_OK;
    if (!head_d || !head_i || !erows) return MPC_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    SlotFetch f{h, head_d, head_i, erows};
    f.derive();
    const RecordShape &sh = f.sh;
    const int fd = sh.fd(), fi = sh.fi(), nr = sh.row_len();
    if (int rc = f.stage_lists()) return rc;
    if (int rc = f.stage_records()) return rc;
    if (h->used_region2) {
        HIP_TRY(h, h->st_hd.ensure((size_t)h->n_opt * fd * sizeof(double)));
        HIP_TRY(h, h->st_hi.ensure((size_t)h->n_opt * fi * sizeof(int32_t)));
        HIP_TRY(h, h->st_pool.ensure((size_t)std::max<long long>(f.pool_rows, 1) * nr * sizeof(double)));
        if (int rc = f.queue_slots(h->st_hd.as<double>(), h->st_hi.as<int32_t>(), h->st_pool.as<double>(), false, nullptr)) return rc;
    }
    if (int rc = f.stage_rlist()) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const int32_t *list = h->st_list.as<int32_t>(), *hi = h->st_hi.as<int32_t>();
    const uint8_t *st = h->st_status.as<uint8_t>();
    const double *hd = h->st_hd.as<double>(), *pool = h->st_pool.as<double>();
    long long wreg = 0, wrow = 0, rpos = 0;
    for (long long w = 0; w < h->n_opt && wreg < cap_regions; ++w) {
        const int cand = list[w];
        const int32_t *src_i = h->used_region2 ? hi + (size_t)w * fi : nullptr;
        double *od = head_d + (size_t)wreg * fd;
        int32_t *oi = head_i + (size_t)wreg * fi;
        const double *rd = nullptr; const int32_t *ri = nullptr;
        int nE = -1;
        if (src_i && src_i[SW_STATUS] == ST_REGION) {                  // a slot the device wrote: copied, its rows rebased
            nE = src_i[SW_NE];
            if (wrow + nE <= cap_rows) {
                std::memcpy(od, hd + (size_t)w * fd, sizeof(double) * fd);
                std::memcpy(oi, src_i, sizeof(int32_t) * fi);
                oi[SW_ROW0] = (int32_t)wrow;
                std::memcpy(erows + (size_t)wrow * nr, pool + (size_t)src_i[SW_ROW0] * nr, sizeof(double) * nE * nr);
            }
        } else if (f.fixed_of(w, cand, src_i && src_i[SW_STATUS] == ST_RETRY, &rpos, &rd, &ri) && rd && st[cand] == ST_REGION) {
            nE = ri[FW_NE];                                             // a fixed record: converted
            if (wrow + nE <= cap_rows) fixed_to_slot(sh, rd, ri, ST_REGION, cand, wrow, od, oi, erows);
        }
        if (nE < 0) continue;
        if (wrow + nE > cap_rows) return fail(h, MPC_ERR_CAPACITY, "row buffer too small (see mpc_compact_strides max_rows)");
        wrow += nE; ++wreg;
    }
    if (n_regions) *n_regions = wreg;
    if (n_rows) *n_rows = wrow;
    return MPC_OK;
}

int mpc_level_regions(mpc_handle *h, double *rec_d, int32_t *rec_i, int64_t *cand_index, int64_t cap) {
    if (!h) return MPC_ERR_INVALID;
    if (!h->level_done) return fail(h, MPC_ERR_STATE, "mpc_level_run has not been called for this frontier");
    if (cap < h->n_regions) return fail(h, MPC_ERR_CAPACITY, "region buffer too small");
    if (h->n_regions == 0) return MPC_OK;
    if (!rec_d || !rec_i) return MPC_ERR_INVALID;
    // fetch in compact form, then expand into the fixed-stride records of the header
    const RecordShape sh = record_shape(h);
    const RecordSizes z = level_record_sizes(h);
    int64_t nreg = 0, nrows = 0;
    std::vector<double> c_hd((size_t)h->n_regions * z.fd), c_er((size_t)std::max<long long>(z.rows_cap, 1) * sh.row_len());
    std::vector<int32_t> c_hi((size_t)h->n_regions * z.fi);
    int rc = mpc_level_regions_compact(h, c_hd.data(), c_hi.data(), h->n_regions, c_er.data(), z.rows_cap, &nreg, &nrows);
    if (rc) return rc;
    for (int64_t w = 0; w < nreg; ++w) {
        const int32_t *si = c_hi.data() + w * z.fi;
        slot_to_fixed(sh, c_hd.data() + w * z.fd, si, c_er.data(), rec_d + w * h->rec_d, rec_i + w * h->rec_i);
        if (cand_index) cand_index[w] = si[SW_CAND];
    }
    return MPC_OK;
}

int mpc_level_regions_device(mpc_handle *h, double *head_d_dev, int32_t *head_i_dev, double *erows_dev, int64_t cap_slots,
                             int64_t cap_rows, int64_t *n_slots, int64_t *n_rows) {
    if (!h) return MPC_ERR_INVALID;
    if (!h->level_done) return fail(h, MPC_ERR_STATE, "mpc_level_run has not been called for this frontier");
    if (n_slots) *n_slots = 0;
    if (n_rows) *n_rows = 0;
    if (h->n_regions == 0 || h->n_opt == 0) return MPC_OK;
    // only the common case lives entirely on the device: every region came from k_region2; otherwise the caller takes the
    // host route (mpc_level_regions_slots)
    if (!h->used_region2 || h->n_rretry > 0 || h->so.active) return fail(h, MPC_ERR_STATE, "records of this level are not all in slot form on the device");
    if (cap_slots < h->n_opt || cap_rows < h->n_erows) return fail(h, MPC_ERR_CAPACITY, "slot / row buffers too small");
    if (!head_d_dev || !head_i_dev || (!erows_dev && h->n_erows > 0)) return MPC_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(head_d_dev, h->headd.p, (size_t)h->n_opt * h->fd * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(head_i_dev, h->headi.p, (size_t)h->n_opt * h->fi * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (h->n_erows > 0) HIP_TRY(h, hipMemcpyAsync(erows_dev, h->epool.p, (size_t)h->n_erows * (h->n_t + 1) * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if (n_slots) *n_slots = h->n_opt;
    if (n_rows) *n_rows = h->n_erows;
    return MPC_OK;
}

// one event per device: "the last k_fetch_many has finished" (recorded on the stream it ran on)
static std::mutex g_fetch_mutex;
static std::map<int, hipEvent_t> g_fetch_event;
// the launch's table, one pair of buffers PER DEVICE: the wait that frees a table for reuse is the same device's previous launch
static std::map<int, DevBuf> g_fetch_tab_dev_of;
static std::map<int, HostBuf> g_fetch_tab_host_of;
static int fetch_many_wait(int device) {
    // Every copy launch waits for the one before it (its table is reused), so the LATEST record of the device's event covers all earlier
    // launches: whoever waits -- from any thread, for any member -- waits for that record (a completed event returns at once).
    hipEvent_t ev = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_fetch_mutex);
        auto it = g_fetch_event.find(device);
        if (it == g_fetch_event.end() || !it->second) return MPC_OK;
        ev = it->second;
    }
    return hipEventSynchronize(ev) == hipSuccess ? MPC_OK : MPC_ERR_HIP;
}
int mpc_fetch_wait(int32_t device) { return fetch_many_wait(device); }

int mpc_level_batch_fetch(mpc_handle **hs, int32_t n_handles, double *const *head_d, int32_t *const *head_i, const int64_t *cap_slots,
                          double *const *erows, const int64_t *cap_rows, int64_t *n_slots, int64_t *n_rows) {
    if (!hs || n_handles < 0 || !head_d || !head_i || !cap_slots || !erows || !cap_rows || !n_slots || !n_rows) return MPC_ERR_INVALID;
    std::vector<FetchEntry> tab;
    mpc_handle *lead = nullptr;
    for (int i = 0; i < n_handles; ++i) {
        mpc_handle *h = hs[i];
        if (!h) return MPC_ERR_INVALID;
        // every record in slot form on the device, nothing streamed, nothing re-solved by the LDS engine: the copy kernel takes the member
        // (round 5: also a member with candidates re-solved by the LDS-engine kernel -- k_rretry_merge writes their records into the slots first)
        const bool merge = h->n_rretry > 0 && h->rretry_rows < 0;
        const RecordShape sh = record_shape(h);
        const long long rows_out = level_record_sizes(h).rows_cap;   // (used where every record is pooled: fast asks for used_region2)
        const bool fast = h->level_done && !h->so.active && h->n_regions > 0 && h->n_opt > 0 && h->used_region2 &&
                          h->n_rretry <= RRETRY_MERGE_MAX && h->n_opt <= 0x7fffffffLL &&
                          (h->n_rretry == 0 || (h->recd.p && h->reci.p && h->retry_list.p && h->epool.cap >= (size_t)rows_out * sh.row_len() * sizeof(double))) &&
                          cap_slots[i] >= h->n_opt && cap_rows[i] >= rows_out && head_d[i] && head_i[i] && (erows[i] || rows_out == 0) &&
                          (!lead || lead->device == h->device);
        void *d_hd = nullptr, *d_hi = nullptr, *d_er = nullptr;
        if (fast && hipHostGetDevicePointer(&d_hd, head_d[i], 0) == hipSuccess && hipHostGetDevicePointer(&d_hi, head_i[i], 0) == hipSuccess &&
            (rows_out == 0 || hipHostGetDevicePointer(&d_er, erows[i], 0) == hipSuccess)) {
            if (!lead) { lead = h; HIP_TRY(lead, hipSetDevice(lead->device)); }
            if (merge) {
                if (h->stream != lead->stream) HIP_TRY(h, hipStreamSynchronize(h->stream));   // (a member that took its level alone: its kernels ran on its own stream)
                RretryMerge a{};
                a.opt_list = h->opt_ptr; a.rlist = h->retry_list.as<int32_t>(); a.status = h->status.as<uint8_t>(); a.recd = h->recd.as<double>(); a.reci = h->reci.as<int32_t>();
                a.headd = h->headd.as<double>(); a.headi = h->headi.as<int32_t>(); a.epool = h->epool.as<double>();
                a.sh = sh; a.n_opt = (int)h->n_opt; a.n_rretry = (int)h->n_rretry; a.row0 = (int)h->n_erows;
                hipLaunchKernelGGL(k_rretry_merge, dim3(1), dim3(256), 0, lead->stream, a);
                HIP_TRY(h, hipGetLastError());
                h->rretry_rows = rows_out;
            }
            tab.push_back({h->headi.p, d_hi, (unsigned long long)h->n_opt * sh.fi() * sizeof(int32_t)});
            tab.push_back({h->headd.p, d_hd, (unsigned long long)h->n_opt * sh.fd() * sizeof(double)});
            if (rows_out > 0) tab.push_back({h->epool.p, d_er, (unsigned long long)rows_out * sh.row_len() * sizeof(double)});
            n_slots[i] = h->n_opt; n_rows[i] = rows_out;
            continue;
        }
        (void)hipGetLastError();
        { const bool dbg = debug_many();
          if (dbg) std::fprintf(stderr, "[many] member %d outside the copy launch: level_done %d streamed %d regions %lld n_opt %lld region2 %d rretry %lld cap_slots %lld erows %lld cap_rows %lld\n", i, (int)h->level_done, (int)h->so.active,
                                (long long)h->n_regions, (long long)h->n_opt, (int)h->used_region2, (long long)h->n_rretry, (long long)cap_slots[i], (long long)h->n_erows, (long long)cap_rows[i]); }
        const int rc = level_regions_slots_impl(h, head_d[i], head_i[i], cap_slots[i], erows[i], cap_rows[i], n_slots + i, n_rows + i, FetchMode::queued_only);
        if (rc != MPC_OK) return rc;
    }
    if (!tab.empty()) {
        HIP_TRY(lead, hipSetDevice(lead->device));
        std::lock_guard<std::mutex> lk(g_fetch_mutex);
        if (g_fetch_event.count(lead->device) && g_fetch_event[lead->device]) HIP_TRY(lead, hipEventSynchronize(g_fetch_event[lead->device]));   // the table of the previous call is free again
        const size_t bytes = tab.size() * sizeof(FetchEntry);
        DevBuf &g_fetch_tab_dev = g_fetch_tab_dev_of[lead->device];
        HostBuf &g_fetch_tab_host = g_fetch_tab_host_of[lead->device];
        HIP_TRY(lead, g_fetch_tab_host.ensure(bytes));
        HIP_TRY(lead, g_fetch_tab_dev.ensure(bytes, lead->stream));
        std::memcpy(g_fetch_tab_host.p, tab.data(), bytes);
        HIP_TRY(lead, hipMemcpyAsync(g_fetch_tab_dev.p, g_fetch_tab_host.p, bytes, hipMemcpyHostToDevice, lead->stream));
        hipLaunchKernelGGL(k_fetch_many, dim3(8, (unsigned)tab.size()), dim3(256), 0, lead->stream, g_fetch_tab_dev.as<FetchEntry>());
        HIP_TRY(lead, hipGetLastError());
        auto &ev = g_fetch_event[lead->device];
        if (!ev) HIP_TRY(lead, pooled_event(&ev, false));
        HIP_TRY(lead, hipEventRecord(ev, lead->stream));
    }
    return MPC_OK;
}

// One launch writes a level's slot records (every record in slot form on the device) into fresh page-locked blocks of lv and raises the
// flag behind head_i; nobody waits here (mpc_solve_level does).  counter: a zero word of device memory nothing else uses before the launch.
static int solve_fetch_slots(mpc_handle *h, mpc_handle::SolveLevel &lv, long long n_opt, int fd, int fi, long long n_erows, size_t b_er,
                             const void *headd, const void *headi, const void *epool, unsigned int *counter) {
    const size_t b_hd = (size_t)n_opt * fd * sizeof(double), b_hi = (size_t)n_opt * fi * sizeof(int32_t);
    if (host_pool_take(b_hd, &lv.hd, nullptr, true) != hipSuccess || host_pool_take(b_hi + 64, &lv.hi, nullptr, true) != hipSuccess ||
        host_pool_take(b_er, &lv.er, nullptr, true) != hipSuccess) return fail(h, MPC_ERR_HIP, "mpc_solve: page-locked memory for a level's region records");
    FetchCopy fc{};
    int32_t *flag = reinterpret_cast<int32_t *>(static_cast<char *>(lv.hi) + ((b_hi + 7) & ~size_t(7)));
    *flag = 0;
    void *d_hd = nullptr, *d_hi = nullptr, *d_er = nullptr;
    if (hipHostGetDevicePointer(&d_hd, lv.hd, 0) != hipSuccess || hipHostGetDevicePointer(&d_hi, lv.hi, 0) != hipSuccess ||
        hipHostGetDevicePointer(&d_er, lv.er, 0) != hipSuccess) return fail(h, MPC_ERR_HIP, "hipHostGetDevicePointer (level records)");
    fc.src[0] = headi; fc.dst[0] = d_hi; fc.bytes[0] = b_hi;
    fc.src[1] = headd; fc.dst[1] = d_hd; fc.bytes[1] = b_hd;
    fc.src[2] = epool; fc.dst[2] = d_er; fc.bytes[2] = (size_t)n_erows * (h->n_t + 1) * sizeof(double);
    fc.counter = counter;
    fc.flag = reinterpret_cast<int32_t *>(static_cast<char *>(d_hi) + ((b_hi + 7) & ~size_t(7)));
    const unsigned long long words = (b_hi + b_hd + fc.bytes[2]) / 4;
    hipLaunchKernelGGL(k_fetch_slots, dim3((unsigned)std::min<unsigned long long>(256, words / 2048 + 1)), dim3(256), 0, h->stream, fc);
    if (hipGetLastError() != hipSuccess) return fail(h, MPC_ERR_HIP, "k_fetch_slots launch");
    lv.ready_flag = flag;
    lv.mode = 2; lv.n_slots = n_opt; lv.n_rows = n_erows; lv.chunk = 0; lv.n_chunks = 0;
    return MPC_OK;
}
