// create.hpp -- the creation of a handle (host code only, no kernels): what create_fill of mpcombi_hip.hip runs for mpc_create.  Included by
// mpcombi_hip.hip alone, below mpc_handle and the helpers it calls (lu_factor, lu_solve_host, make_layout, apply_layout, side_streams,
// untimed_events, the pools, lp_batch, setup_launch): the translation unit stays one.
//
// CreateRun is the creation's context: it lives on create_fill's stack, is built once per handle and owns nothing.  Its member functions
// are the stages, in the order create_fill calls them (DESIGN 3.1 has the map).  What a stage leaves for a later one is a member, and each
// member says who sets it and who reads it.  Creation runs once per binary fixation of a mixed-integer program: no stage adds a
// synchronisation, an LP batch, a device allocation or a copy to what the one function did (6 hipStreamSynchronize, at most 3 lp_batch
// calls, 9 device allocations, 6 host-to-device copies).  Errors go to the thread-local text (fail(nullptr, ...)): the caller destroys
// the handle.
#pragma once

namespace {   // (internal linkage: the library exports the C ABI and nothing of this)

struct CreateRun {
    // ---- constants of the creation (set by the constructor) -------------------------------------------------------------------------------
    const mpc_problem *const p;     // the caller's program
    const int32_t device;
    void *const stream;             // the caller's stream (nullptr: one of the pool's)
    mpc_handle *const h;            // the fresh handle every stage fills
    const int nx, nt, nc, ne, ntc;  // n_x, n_t, n_c, n_eq, n_tc of the program
    const int nr;                   // n_t + 1: columns of a parametric right-hand side
    const int cols, rows_x;         // 1 + n_x + n_t columns and n_c + n_tc rows of the base rows
    // ---- host copies of what goes into the blocks ------------------------------------------------------------------------------------------
    std::vector<double> base;       // set by base_rows: [b | A | -F ; b_t | 0 | A_t]; read by base_dictionary, pack_blocks
    std::vector<double> d0, d0T;    // set by base_dictionary: the pre-crashed dictionary and its transpose (empty: none); read by pack_blocks, problem_views
    std::vector<int> d0_rows, d0_cols;   // set by base_dictionary: its row / column maps; read by problem_views
    std::vector<double> tv_theta, tv_minv, tv_rows;   // set by theta_vertex: vertex of the parameter set, inverse of its tight rows, the other rows in its
                                    // coordinates (empty: no vertex); read by pack_blocks, problem_views, theta_blocks, theta_open
    std::vector<int> tv_tight;      // set by theta_vertex: the tight rows; read by problem_views
    // offsets (doubles) of the read-only blocks in h->blocks; set by pack_blocks; read by schur_setup, problem_views, theta_blocks
    struct Offsets { size_t A, b, F, c, H, Q, At, bt, W, UV, Gt, X0H, AAT, ATr, Wr, UVr, AATr, Me, Ne, gE, base, d0, d0T, tvt, tvm, tvr; } o{};
    std::vector<double> host;       // set by pack_blocks: the blocks as uploaded (pageable: it has to outlive the copy, which schur_setup's synchronisation ends)
    bool want_elim = false;         // set by pack_blocks: the blocks with the equality rows eliminated are asked for; read by schur_setup
    std::vector<double> UV, UVr;    // set by schur_setup: host copies of the set-up kernel's UV / UVr; read by theta_blocks
    int mode = 1;                   // set by schur_setup: kkt_mode (0: Schur blocks valid, 1: KKT system); read by problem_views, lds_layouts, theta_blocks, register_path
    bool elim_ok = false;           // set by schur_setup: the eliminated blocks are valid; read by theta_blocks
    // ---- views and layouts ------------------------------------------------------------------------------------------------------------------
    const double *d = nullptr;      // set by problem_views: h->blocks on the device; read by theta_blocks
    DevProblem P{};                 // set by problem_views, lds_layouts (kmax, ld_x, ld_t): the view every layout starts from; read by lds_layouts, register_path, theta_blocks, region2_view
    int kmax = 0, rows_t = 0;       // set by lds_layouts: min(n_c, n_x); region rows n_c - n_eq + n_tc; read by register_path, region2_view
    int size_K = 0, size_L = 0, size_X = 0;   // set by lds_layouts: doubles of the K, L and X areas; read by register_path, region2_view
    int tsel = -1, slots_t = 0;     // set by register_path: n_theta class of the instantiations, slots of the theta rows; read by theta_blocks, region2_view
    int NTP = 0, LS = 0;            // set by register_path: compile-time NT of the class, row stride NT + 1; read by theta_blocks, region2_view
    // ---- bounding box of the parameter set (theta_box: at most once per creation) -------------------------------------------------------
    bool box_done = false;          // set by theta_box; read by theta_blocks, theta_open
    bool box_open = false;          // set by theta_box: some side is infinite (the batch failed or an LP was not optimal); read by theta_blocks, theta_open
    std::vector<double> box_lo, box_hi;   // set by theta_box: the sides, widened a little (-inf / +inf: open); read by theta_blocks

    CreateRun(const mpc_problem *p_, int32_t device_, void *stream_, mpc_handle *h_)
        : p(p_), device(device_), stream(stream_), h(h_), nx(p_->n_x), nt(p_->n_t), nc(p_->n_c), ne(p_->n_eq), ntc(p_->n_tc), nr(p_->n_t + 1),
          cols(1 + p_->n_x + p_->n_t), rows_x(p_->n_c + p_->n_tc) {}

    // ==== stages ============================================================================================================================
    // device, CU count, clock rate, streams and events from the pools (mpc_destroy returns them by the same two lists), the environment
    int sync_objects() {
        h->device = device;
        HIP_TRY(nullptr, hipSetDevice(device));
        h->n_cu = cu_count(device);
        { int khz = 0; if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) h->wall_khz = khz; }
        if (stream) { h->stream = reinterpret_cast<hipStream_t>(stream); h->own_stream = false; }
        else { HIP_TRY(nullptr, pooled_stream(&h->stream)); h->own_stream = true; }
        for (auto &e : h->ev) HIP_TRY(nullptr, pooled_event(&e, true));
        for (auto &e : h->kev) HIP_TRY(nullptr, pooled_event(&e, true));
        for (hipStream_t *s : side_streams(h)) HIP_TRY(nullptr, pooled_stream(s));
        for (hipEvent_t *e : untimed_events(h)) HIP_TRY(nullptr, pooled_event(e, false));
        h->kn = Knobs::from_env();
        h->n_x = nx; h->n_t = nt; h->n_c = nc; h->n_eq = ne; h->n_tc = ntc; h->is_qp = p->Q != nullptr;
        h->mw = nc <= 64 * MPC_MASK_WORDS ? MPC_MASK_WORDS : 4;
        return MPC_OK;
    }

    void base_rows() {
        base.assign((size_t)rows_x * cols, 0.0);
        for (int i = 0; i < nc; ++i) {
            base[(size_t)i * cols] = p->b[i];
            for (int j = 0; j < nx; ++j) base[(size_t)i * cols + 1 + j] = p->A[(size_t)i * nx + j];
            for (int j = 0; j < nt; ++j) base[(size_t)i * cols + 1 + nx + j] = -p->F[(size_t)i * nt + j];
        }
        for (int i = 0; i < ntc; ++i) {
            base[(size_t)(nc + i) * cols] = p->b_t[i];
            for (int j = 0; j < nt; ++j) base[(size_t)(nc + i) * cols + 1 + nx + j] = p->A_t[(size_t)i * nt + j];
        }
    }

    // ---- pre-crashed dictionary D0 of the (x,theta) LP (see xtheta_from_vertex in kernels.hpp) --------------------
    // A feasible vertex of the base polytope {A x - F theta <= b (first n_eq rows =), A_t theta <= b_t} is found once by
    // the device simplex; the dictionary at that vertex is then rebuilt from the original rows by a fresh LU, so its
    // entries carry factorisation-level accuracy, not the accumulated error of the pivot sequence.
    int base_dictionary() {
        const int nv = nx + nt;
        std::vector<double> Alp((size_t)rows_x * nv), blp(rows_x);
        for (int i = 0; i < rows_x; ++i) { blp[i] = base[(size_t)i * cols]; for (int j = 0; j < nv; ++j) Alp[(size_t)i * nv + j] = base[(size_t)i * cols + 1 + j]; }
        std::vector<uint8_t> eqf(rows_x, 0);
        for (int i = 0; i < ne; ++i) eqf[i] = 1;
        std::vector<int32_t> tight(rows_x, 0);
        int32_t lp_status = -1;
        int rc0 = rows_x > nv ? lp_batch(device, 1, rows_x, nv, Alp.data(), 1, blp.data(), 1, nullptr, 1, eqf.data(), &lp_status, nullptr, nullptr, nullptr, tight.data()) : MPC_ERR_INVALID;
        HIP_TRY(nullptr, hipSetDevice(device));
        std::vector<int> B;
        for (int i = 0; i < rows_x; ++i) if (tight[i]) B.push_back(i);
        bool ok = rc0 == MPC_OK && lp_status == LP_OPTIMAL && (int)B.size() == nv;
        std::vector<double> MT;
        std::vector<int> perm;
        if (ok) {
            MT.assign((size_t)nv * nv, 0.0);  // M^T, M = rows B of [A | -F ; 0 | A_t]
            for (int r = 0; r < nv; ++r) for (int j = 0; j < nv; ++j) MT[(size_t)j * nv + r] = Alp[(size_t)B[r] * nv + j];
            ok = lu_factor(MT, nv, perm);
        }
        if (ok) {
            std::vector<char> inB(rows_x, 0);
            for (int r : B) inB[r] = 1;
            std::vector<int> colpos;  // positions in B of the inequality rows (the alive nonbasic columns)
            for (int r = 0; r < nv; ++r) if (B[r] >= ne) { colpos.push_back(r); d0_cols.push_back(B[r]); }
            std::vector<double> y(nv);
            const int nc0 = (int)d0_cols.size();
            for (int i = 0; i < rows_x && ok; ++i) {
                if (inB[i]) continue;
                lu_solve_host(MT, perm, nv, &Alp[(size_t)i * nv], y.data());  // y = a_i M^-1
                double beta = blp[i];
                for (int r = 0; r < nv; ++r) beta -= y[r] * blp[B[r]];
                if (beta < -1e-7) ok = false;
                d0_rows.push_back(i);
                d0.push_back(beta);
                for (int q = 0; q < nc0; ++q) d0.push_back(-y[colpos[q]]);
            }
        }
        if (!ok) { d0.clear(); d0_rows.clear(); d0_cols.clear(); }
        if (h->kn.debug_create)
            std::fprintf(stderr, "[mpc] create: base vertex rc %d status %d, %d tight rows of n_x + n_t = %d -> pre-crashed dictionary %s\n", rc0, (int)lp_status,
                         (int)B.size(), nv, ok ? "built" : "NOT built (no register-resident fast path for this program)");
        if (!d0.empty()) {
            const int mr = (int)d0_rows.size(), cc = 1 + (int)d0_cols.size();
            d0T.assign((size_t)mr * cc, 0.0);
            for (int i = 0; i < mr; ++i) for (int j = 0; j < cc; ++j) d0T[(size_t)j * mr + i] = d0[(size_t)i * cc + j];
        }
        return MPC_OK;
    }

    // ---- vertex of the parameter polytope {A_t theta <= b_t} (kernels2.hpp) ----------------------------------------
    int theta_vertex() {
        bool ok = ntc >= nt;
        std::vector<int32_t> tight(std::max(ntc, 1), 0);
        int32_t lp_status = -1;
        if (ok) {
            std::vector<uint8_t> eqf(ntc, 0);
            if (ntc == nt) {
                // Exactly n_theta rows (round 6): if they are independent (the LU below decides) their common point is the set's only vertex
                // -- a pointed cone, e.g. the lower bounds of theta that a presolve leaves when the main rows imply the upper ones
                // (profiles/r05_sweep.json: mpqp_10_2_20 / _30 ran on the LDS-engine kernels for want of this case).
                for (int i = 0; i < ntc; ++i) tight[i] = 1;
                lp_status = LP_OPTIMAL;
            } else {
                int rc0 = lp_batch(device, 1, ntc, nt, p->A_t, 1, p->b_t, 1, nullptr, 1, eqf.data(), &lp_status, nullptr, nullptr, nullptr, tight.data());
                HIP_TRY(nullptr, hipSetDevice(device));
                ok = rc0 == MPC_OK && lp_status == LP_OPTIMAL;
            }
        }
        std::vector<int> B;
        for (int i = 0; i < ntc && ok; ++i) if (tight[i]) B.push_back(i);
        ok = ok && (int)B.size() == nt;
        std::vector<double> M, MTf;
        std::vector<int> perm;
        if (ok) {
            M.assign((size_t)nt * nt, 0.0);
            for (int r = 0; r < nt; ++r) for (int j = 0; j < nt; ++j) M[(size_t)r * nt + j] = p->A_t[(size_t)B[r] * nt + j];
            std::vector<double> LU(M);
            ok = lu_factor(LU, nt, perm);
            if (ok) {
                tv_minv.assign((size_t)nt * nt, 0.0);
                std::vector<double> e(nt), x(nt);
                for (int j = 0; j < nt; ++j) {   // column j of M^-1
                    std::fill(e.begin(), e.end(), 0.0); e[j] = 1.0;
                    lu_solve_host(LU, perm, nt, e.data(), x.data());
                    for (int t = 0; t < nt; ++t) tv_minv[(size_t)t * nt + j] = x[t];
                }
                std::vector<double> bB(nt);
                for (int r = 0; r < nt; ++r) bB[r] = p->b_t[B[r]];
                tv_theta.assign(nt, 0.0);
                lu_solve_host(LU, perm, nt, bB.data(), tv_theta.data());
                std::vector<char> inB(ntc, 0);
                for (int r : B) inB[r] = 1;
                for (int i = 0; i < ntc; ++i) {
                    if (inB[i]) continue;
                    double mx = 0; for (int t = 0; t < nt; ++t) mx = std::max(mx, std::fabs(p->A_t[(size_t)i * nt + t]));
                    double sc = 1.0;
                    if (mx > 1e-8) { int ex; std::frexp(mx, &ex); sc = std::ldexp(1.0, -ex); }
                    double beta = p->b_t[i] * sc;
                    for (int t = 0; t < nt; ++t) beta -= (mx > 1e-8 ? p->A_t[(size_t)i * nt + t] * sc : 0.0) * tv_theta[t];
                    tv_rows.push_back(beta);
                    for (int j = 0; j < nt; ++j) {
                        double acc = 0; for (int t = 0; t < nt; ++t) acc += (mx > 1e-8 ? p->A_t[(size_t)i * nt + t] * sc : 0.0) * tv_minv[(size_t)t * nt + j];
                        tv_rows.push_back(-acc);
                    }
                }
            }
        }
        if (!ok) { tv_theta.clear(); tv_minv.clear(); tv_rows.clear(); } else tv_tight = B;
        return MPC_OK;
    }

    // ---- one device allocation for every read-only block -------------------------------------------------
    int pack_blocks() {
        auto put = [&](const double *src, size_t cnt) { size_t off = host.size(); host.insert(host.end(), src, src + cnt); while (host.size() % 2) host.push_back(0.0); return off; };
        std::vector<double> zeros((size_t)std::max(nx * nx, 1), 0.0);
        o.A = put(p->A, (size_t)nc * nx); o.b = put(p->b, nc); o.F = put(p->F, (size_t)nc * nt); o.c = put(p->c, nx); o.H = put(p->H, (size_t)nx * nt);
        o.Q = put(p->Q ? p->Q : zeros.data(), (size_t)nx * nx);
        o.At = put(ntc ? p->A_t : zeros.data(), (size_t)std::max(ntc * nt, 1)); o.bt = put(ntc ? p->b_t : zeros.data(), std::max(ntc, 1));
        // the blocks the set-up kernel fills are reserved at full size (zero until then)
        auto reserve = [&](size_t cnt) { const std::vector<double> z(std::max<size_t>(cnt, 1), 0.0); return put(z.data(), z.size()); };
        const bool dev_schur = p->Q != nullptr;
        o.W = reserve(dev_schur ? (size_t)nc * nc : 1); o.UV = reserve(dev_schur ? (size_t)nc * nr : 1);
        o.Gt = reserve(dev_schur ? (size_t)nc * nx : 1); o.X0H = reserve(dev_schur ? (size_t)nx * nr : 1);
        o.AAT = reserve((size_t)nc * nc);
        std::vector<double> ATr((size_t)std::max(nx * nc, 1), 0.0);      // A transposed (k_region2's row build reads a column of A per step)
        for (int i = 0; i < nc; ++i) for (int l = 0; l < nx; ++l) ATr[(size_t)l * nc + i] = p->A[(size_t)i * nx + l];
        o.ATr = put(ATr.data(), ATr.size());
        // equality rows eliminated from the Schur blocks (setup_mfma.hpp): lets k_kkt_thread take active sets of ne + (1..8) rows
        want_elim = ne > 0 && dev_schur && !h->kn.no_eq_elim;
        o.Wr = reserve(want_elim ? (size_t)nc * nc : 1); o.UVr = reserve(want_elim ? (size_t)nc * nr : 1);
        o.AATr = reserve(want_elim ? (size_t)nc * nc : 1); o.Me = reserve(want_elim ? (size_t)ne * nr : 1);
        o.Ne = reserve(want_elim ? (size_t)ne * nc : 1); o.gE = reserve(want_elim ? (size_t)2 * ne : 1);
        o.base = put(base.data(), base.size());
        o.d0 = put(d0.empty() ? zeros.data() : d0.data(), d0.empty() ? 1 : d0.size());
        o.d0T = put(d0T.empty() ? zeros.data() : d0T.data(), d0T.empty() ? 1 : d0T.size());
        o.tvt = put(tv_theta.empty() ? zeros.data() : tv_theta.data(), tv_theta.empty() ? 1 : tv_theta.size());
        o.tvm = put(tv_minv.empty() ? zeros.data() : tv_minv.data(), tv_minv.empty() ? 1 : tv_minv.size());
        o.tvr = put(tv_rows.empty() ? zeros.data() : tv_rows.data(), tv_rows.empty() ? 1 : tv_rows.size());
        h->o_elim[0] = o.Wr; h->o_elim[1] = o.UVr; h->o_elim[2] = o.AATr; h->o_elim[3] = o.Me; h->o_elim[4] = o.Ne; h->o_elim[5] = o.gE;
        HIP_TRY(nullptr, h->blocks.ensure(host.size() * sizeof(double), h->stream));
        HIP_TRY(nullptr, hipMemcpyAsync(h->blocks.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        return MPC_OK;
    }

    // ---- the dense Hessian factor and the one-off Schur blocks W = A Q^-1 A', UV, G', X0H, A A' on the matrix cores (setup_mfma.hip) ----
    int schur_setup() {
        double *db = h->blocks.as<double>();
        SetupJob job{};
        job.nx = nx; job.nt = nt; job.nc = nc; job.NP = setup_pad16(nx); job.MP = setup_pad16(nc); job.RP = setup_pad16(nr);
        job.A = db + o.A; job.b = db + o.b; job.F = db + o.F; job.c = db + o.c; job.H = db + o.H; job.Q = p->Q ? db + o.Q : nullptr;
        job.W = db + o.W; job.UV = db + o.UV; job.Gt = db + o.Gt; job.X0H = db + o.X0H; job.AAT = db + o.AAT;
        DevBuf work, jobbuf;
        const size_t job_bytes = (sizeof(SetupJob) + 15) & ~size_t(15);
        hipError_t e1 = work.ensure(setup_work_doubles(nx, nt, nc) * sizeof(double), h->stream);
        hipError_t e2 = e1 == hipSuccess ? jobbuf.ensure(job_bytes + 16, h->stream) : e1;
        int flag = 1, flag_e = 1;
        if (e2 == hipSuccess) {
            job.work = work.as<double>();
            job.flag = reinterpret_cast<int *>(jobbuf.as<char>() + job_bytes);
            if (want_elim) {
                job.ne = ne; job.Wr = db + o.Wr; job.UVr = db + o.UVr; job.AATr = db + o.AATr; job.Me = db + o.Me; job.Ne = db + o.Ne; job.gE = db + o.gE;
                job.flag_e = job.flag + 1;
            }
            e2 = hipMemcpyAsync(jobbuf.p, &job, sizeof(SetupJob), hipMemcpyHostToDevice, h->stream);
            if (e2 == hipSuccess) e2 = setup_launch(jobbuf.as<SetupJob>(), 1, h->stream);
            if (e2 == hipSuccess) e2 = hipMemcpyAsync(&flag, job.flag, sizeof(int), hipMemcpyDeviceToHost, h->stream);
            if (e2 == hipSuccess && p->Q) { UV.assign((size_t)nc * nr, 0.0); e2 = hipMemcpyAsync(UV.data(), job.UV, UV.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream); }
            if (e2 == hipSuccess && want_elim) {
                UVr.assign((size_t)nc * nr, 0.0);
                e2 = hipMemcpyAsync(UVr.data(), job.UVr, UVr.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
                if (e2 == hipSuccess) e2 = hipMemcpyAsync(&flag_e, job.flag_e, sizeof(int), hipMemcpyDeviceToHost, h->stream);
            }
            if (e2 == hipSuccess) e2 = hipStreamSynchronize(h->stream);
        }
        work.release(); jobbuf.release();   // the stream has been synchronised (or nothing was queued)
        if (e2 != hipSuccess) return fail(nullptr, MPC_ERR_HIP, std::string("MFMA set-up kernel: ") + hipGetErrorString(e2));
        mode = (p->Q && flag == 0) ? 0 : 1;
        elim_ok = want_elim && mode == 0 && flag_e == 0;
        h->elim_ok = elim_ok;
        HIP_TRY(nullptr, hipStreamSynchronize(h->stream));
        h->kkt_mode = mode;
        return MPC_OK;
    }

    // the view of the program every kernel starts from, and the integer maps of the dictionary and the vertex
    int problem_views() {
        d = h->blocks.as<double>();
        P.n_x = nx; P.n_t = nt; P.n_c = nc; P.n_eq = ne; P.n_tc = ntc; P.is_qp = h->is_qp; P.kkt_mode = mode;
        P.A = d + o.A; P.b = d + o.b; P.F = d + o.F; P.c = d + o.c; P.H = d + o.H; P.Q = d + o.Q; P.A_t = d + o.At; P.b_t = d + o.bt;
        P.W = d + o.W; P.UV = d + o.UV; P.Gt = d + o.Gt; P.X0H = d + o.X0H; P.base = d + o.base; P.AAT = d + o.AAT; P.AT = d + o.ATr;
        P.d0T = d + o.d0T; P.tv_theta = d + o.tvt; P.tv_minv = d + o.tvm; P.tv_rows = d + o.tvr;
        P.has_tv = tv_theta.empty() ? 0 : 1; P.n_tpre = tv_theta.empty() ? 0 : ntc - nt;
        P.d0 = d + o.d0; P.has_d0 = d0.empty() ? 0 : 1; P.n_d0r = (int)d0_rows.size(); P.n_d0c = (int)d0_cols.size();
        std::vector<int> maps(d0_rows);
        maps.insert(maps.end(), d0_cols.begin(), d0_cols.end());
        maps.insert(maps.end(), tv_tight.begin(), tv_tight.end());
        if (maps.empty()) maps.push_back(0);
        HIP_TRY(nullptr, h->iblocks.ensure(maps.size() * sizeof(int), h->stream));
        HIP_TRY(nullptr, hipMemcpyAsync(h->iblocks.p, maps.data(), maps.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(nullptr, hipStreamSynchronize(h->stream));
        P.d0_rows = h->iblocks.as<int>();
        P.d0_cols = h->iblocks.as<int>() + d0_rows.size();
        P.tv_tight = h->iblocks.as<int>() + d0_rows.size() + d0_cols.size();
        return MPC_OK;
    }

    // ---- LDS layouts ---------------------------------------------------------------------------------------
    int lds_layouts() {
        kmax = std::min(nc, nx);
        rows_t = nc - ne + ntc;
        P.kmax = kmax;
        P.ld_x = odd_at_least(nx + nt + 3);
        P.ld_t = odd_at_least(nt + 4);
        size_K = mode == 0 ? std::max(kmax * kmax + kmax, kmax * nx) : std::max({(nx + kmax) * (nx + kmax) + (nx + kmax) * nr, kmax * nx, nx * nx});
        size_L = std::max(kmax * nr, 1); size_X = nx * nr;
        const int T_v = std::max((rows_x + 1) * P.ld_x, (rows_t + 1) * P.ld_t);
        const int T_r = std::max((rows_t + 2) * P.ld_t, rows_t * nr);
        const Layout lv = make_layout(T_v, size_K, size_L, 0, mode == 1 ? size_X : 0, kmax, nc, std::max(P.ld_x, P.ld_t), rows_x + 1, rows_t);
        const Layout lr = make_layout(T_r, size_K, size_L, rows_t * nr, size_X, kmax, nc, P.ld_t, rows_t + 2, rows_t);
        h->Pv = P; apply_layout(h->Pv, lv); h->lds_v = lv.bytes;
        h->Pr = P; apply_layout(h->Pr, lr); h->lds_r = lr.bytes;
        if (h->lds_v > 160 * 1024 || h->lds_r > 160 * 1024) return fail(nullptr, MPC_ERR_INVALID, "problem does not fit the 160 KiB LDS of one CU");
        if (h->lds_v > 48 * 1024) HIP_TRY(nullptr, hipFuncSetAttribute(reinterpret_cast<const void *>(k_verdict), hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_v));
        if (h->lds_r > 48 * 1024) {
            HIP_TRY(nullptr, hipFuncSetAttribute(reinterpret_cast<const void *>(k_region<RG_FULL>), hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_r));
            HIP_TRY(nullptr, hipFuncSetAttribute(reinterpret_cast<const void *>(k_region<RG_FACET>), hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_r));
            HIP_TRY(nullptr, hipFuncSetAttribute(reinterpret_cast<const void *>(k_region<RG_ASSEMBLE>), hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_r));
        }
        h->grid_v = h->n_cu * waves_per_cu(h->lds_v);
        h->grid_r = h->n_cu * waves_per_cu(h->lds_r);
        return MPC_OK;
    }

    // bounding box of the parameter polytope: 2 n_t LPs on the device (an unbounded direction gives +-inf).  The register-resident
    // kernels screen with it (theta_blocks) and theta_open asks it whether a set with a vertex is an open cone: whoever comes first runs it.
    int theta_box() {
        std::vector<double> cc((size_t)2 * nt * nt, 0.0), obj(2 * nt, 0.0);
        for (int t = 0; t < nt; ++t) { cc[(size_t)(2 * t) * nt + t] = 1.0; cc[(size_t)(2 * t + 1) * nt + t] = -1.0; }
        std::vector<uint8_t> eqz((size_t)2 * nt * ntc, 0);
        std::vector<int32_t> stt(2 * nt, -1);
        const int rcb = lp_batch(device, 2 * nt, ntc, nt, p->A_t, 1, p->b_t, 1, cc.data(), 0, eqz.data(), stt.data(), nullptr, obj.data(), nullptr, nullptr);
        HIP_TRY(nullptr, hipSetDevice(device));
        box_lo.assign(nt, 0.0); box_hi.assign(nt, 0.0);
        for (int t = 0; t < nt; ++t) {
            const bool ok_lo = rcb == MPC_OK && stt[2 * t] == LP_OPTIMAL, ok_hi = rcb == MPC_OK && stt[2 * t + 1] == LP_OPTIMAL;
            // the LP optimum carries the simplex tolerance: widen the box a little (the screen only needs an outer box)
            const double lo = ok_lo ? obj[2 * t] : -INFINITY, hi = ok_hi ? -obj[2 * t + 1] : INFINITY;
            box_open = box_open || !ok_lo || !ok_hi;
            const double pad = 1e-6 * (1.0 + std::max(std::fabs(ok_lo ? lo : 0.0), std::fabs(ok_hi ? hi : 0.0)));
            box_lo[t] = lo - pad;
            box_hi[t] = hi + pad;
        }
        box_done = true;
        return MPC_OK;
    }

    // zero-padded blocks of k_theta2 (ThetaArgs) for its compile-time NT
    int theta_blocks() {
        std::vector<double> tb;
        const size_t oUVp = tb.size(); tb.resize(tb.size() + (size_t)nc * LS, 0.0);
        if (mode == 0) for (int i = 0; i < nc; ++i) for (int t = 0; t < nr; ++t) tb[oUVp + (size_t)i * LS + t] = UV[(size_t)i * nr + t];
        const size_t oUVrp = tb.size();
        if (elim_ok) {
            tb.resize(tb.size() + (size_t)nc * LS, 0.0);
            for (int i = 0; i < nc; ++i) for (int t = 0; t < nr; ++t) tb[oUVrp + (size_t)i * LS + t] = UVr[(size_t)i * nr + t];
        }
        const size_t otvp = tb.size(); tb.resize(tb.size() + (size_t)NTP * NTP + 3 * NTP, 0.0);
        for (int t = 0; t < nt; ++t) for (int j = 0; j < nt; ++j) tb[otvp + (size_t)t * NTP + j] = tv_minv[(size_t)t * nt + j];
        for (int t = 0; t < nt; ++t) tb[otvp + (size_t)NTP * NTP + t] = tv_theta[t];
        { const int rcb = theta_box(); if (rcb != MPC_OK) return rcb; }
        for (int t = 0; t < nt; ++t) {
            tb[otvp + (size_t)NTP * NTP + NTP + t] = box_lo[t];
            tb[otvp + (size_t)NTP * NTP + 2 * NTP + t] = box_hi[t];
        }
        const int npre = ntc - nt;
        const size_t otvr = tb.size(); tb.resize(tb.size() + (size_t)std::max(npre, 1) * LS, 0.0);
        for (int i = 0; i < npre; ++i) for (int t = 0; t < nr; ++t) tb[otvr + (size_t)i * LS + t] = tv_rows[(size_t)i * nr + t];
        HIP_TRY(nullptr, h->theta_blocks.ensure(tb.size() * sizeof(double), h->stream));
        HIP_TRY(nullptr, hipMemcpyAsync(h->theta_blocks.p, tb.data(), tb.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(nullptr, hipStreamSynchronize(h->stream));
        const double *tbd = h->theta_blocks.as<double>();
        h->targs.box_finite = (box_done && !box_open && !h->kn.kkt_box_select) ? 1 : 0;   // (MPC_KKT_BOX_SELECT=1: the select form of the screen's row test on every program; tests)
        h->targs.W = P.W; h->targs.UVp = tbd + oUVp; h->targs.tvp = tbd + otvp; h->targs.tv_rows = tbd + otvr; h->targs.chunk = 1;
        h->targs.ne = elim_ok ? ne : 0;
        // MPC_TH_DIV (work items per wavefront of k_theta2, default 4; 0 = round-3 behaviour) / MPC_TH_MAXW (waves per SIMD, default 2)
        h->targs.wave_div = h->kn.th_div;
        h->targs.wave_max = h->kn.th_maxw * 4 * h->n_cu;
        if (h->targs.wave_div <= 0) { h->targs.wave_div = 0; h->targs.wave_max = 0; }
        h->targs.Wr = elim_ok ? d + o.Wr : P.W; h->targs.UVrp = elim_ok ? tbd + oUVrp : h->targs.UVp; h->targs.AATr = elim_ok ? d + o.AATr : P.AAT;
        h->targs.Me = d + o.Me; h->targs.Ne = d + o.Ne; h->targs.gE = d + o.gE;
        return MPC_OK;
    }

    // k_region2: all rows_t region rows plus the cost row, n_t >= 2 (the one-parameter variant stays on k_region)
    int region2_view() {
        const int slots_r = rows_t + 1 <= 64 ? 1 : (rows_t + 1 <= 128 ? 2 : 0);
        if (!(nt >= 2 && slots_r)) return MPC_OK;
        h->fast_r = tsel * 2 + (slots_r - 1);
        // (T: the staged [tv_minv | tv_theta | box] block, round 6)
        const Layout l2 = make_layout(NTP * NTP + 3 * NTP, std::max(size_K, nt * (2 * nt + 1)), size_L, rows_t * nr, size_X, kmax, nc, nt + 2, 2, rows_t);
        h->Pr2 = P; apply_layout(h->Pr2, l2); h->lds_r2 = l2.bytes;
        h->Pr2.tvp = h->targs.tvp;
        h->grid_r2 = h->n_cu * std::min(4 * (slots_r >= 2 ? 2 : R2W), waves_per_cu(h->lds_r2));   // waves per SIMD of the launch bounds
        HIP_TRY(nullptr, h->pr2_dev.ensure(sizeof(DevProblem), h->stream));
        HIP_TRY(nullptr, hipMemcpyAsync(h->pr2_dev.p, &h->Pr2, sizeof(DevProblem), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(nullptr, hipStreamSynchronize(h->stream));
        return MPC_OK;
    }

    // fast path (k_verdict2): needs the theta vertex, the pre-crashed dictionary and sizes inside the instantiations
    int register_path() {
        const int rows_th = rows_t - nt, rows_d0 = P.n_d0r;
        slots_t = rows_th <= 64 ? 1 : (rows_th <= 128 ? 2 : 0);
        const int slots_x = rows_d0 <= 64 ? 1 : (rows_d0 <= 128 ? 2 : 0);
        tsel = nt <= 4 ? 0 : (nt <= 8 ? 1 : (nt <= 10 ? 2 : -1));   // kernels are instantiated for n_theta <= 4, 8, 10
        const int xsel = P.n_d0c <= 14 ? 0 : (P.n_d0c <= 30 ? 1 : -1);
        if (h->kn.debug_create)
            std::fprintf(stderr, "[mpc] create: vertex of the parameter set %d, dictionary %d (rows %d, columns %d), theta rows %d -> slots %d / %d, n_theta class %d, column class %d: register-resident kernels %s\n",
                         (int)P.has_tv, (int)P.has_d0, rows_d0, (int)P.n_d0c, rows_th, slots_t, slots_x, tsel, xsel,
                         (P.has_tv && P.has_d0 && slots_t && slots_x && tsel >= 0 && xsel >= 0) ? "ON" : "OFF (LDS-engine kernels)");
        if (!(P.has_tv && P.has_d0 && slots_t && slots_x && tsel >= 0 && xsel >= 0)) return MPC_OK;
        h->fast = 1;
        h->fast_t = tsel * 2 + (slots_t - 1);
        h->fast_x = xsel * 2 + (slots_x - 1);
        if (xsel >= 1) h->kn.x2_wpc = std::min(h->kn.x2_wpc, 4 * X2_WAVES);   // the 32-column instantiations of k_x2 are built for two wavefronts per SIMD
        NTP = tsel == 0 ? 4 : (tsel == 1 ? 8 : 10); LS = NTP + 1;
        { const int rc = theta_blocks(); if (rc != MPC_OK) return rc; }
        const Layout lf = make_layout(NTP * NTP + 3 * NTP + kmax * LS, size_K, size_L, 0, mode == 1 ? size_X : 0, kmax, nc, 2, 2, 2);
        h->Pf = P; apply_layout(h->Pf, lf); h->lds_f = lf.bytes;
        h->targs.cbuf_off = 0;
        if (slots_t == 2) {   // scratch of the live-row compaction of k_theta2<., 2>: 64 rows of NT+4 doubles and 2 ints
            h->targs.cbuf_off = h->lds_f / 8;
            h->lds_f += 64 * (NTP + 4) * 8 + 64 * 2 * 4;
            h->lds_f = (h->lds_f + 15) & ~15;
        }
        h->grid_f = h->n_cu * std::min(16, waves_per_cu(h->lds_f));
        HIP_TRY(nullptr, h->pf_dev.ensure(sizeof(DevProblem), h->stream));
        HIP_TRY(nullptr, hipMemcpyAsync(h->pf_dev.p, &h->Pf, sizeof(DevProblem), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(nullptr, hipStreamSynchronize(h->stream));
        return region2_view();
    }

    // ---- is the parameter set open in some direction?  (then the reference's optimality LP can be unbounded: k_recession) -------------
    int theta_open() {
        bool open = false;
        if (nc == ne) open = true;                                     // no multiplier / slack row at all bounds t (the base set)
        else if (nt > 0 && (ntc == 0 || tv_theta.empty())) open = true;   // no row, or no vertex: the set contains a line (or the search failed: the test is always safe)
        else if (nt > 0) {
            // a vertex, but maybe an open cone: the bounding box (2 n_t LPs on the device, as for the register-resident kernels)
            if (!box_done) { const int rcb = theta_box(); if (rcb != MPC_OK) return rcb; }
            open = box_open;
        }
        h->theta_open = open;
        if (h->kn.debug_create) std::fprintf(stderr, "[mpc] create: parameter set %s\n", open ? "OPEN in some direction (k_recession behind the verdict stages)" : "bounded");
        return MPC_OK;
    }

    int records_and_counters() {
        h->rec_d = record_shape(h, 0).rec_d();   // (the fixed record does not depend on the cardinality)
        h->rec_i = record_shape(h, 0).rec_i();
        HIP_TRY(nullptr, h->ctr.ensure(sizeof(LevelCounters), h->stream));
        HIP_TRY(nullptr, h->scratch.ensure(256, h->stream));
        void *hp = nullptr, *dp = nullptr;
        HIP_TRY(nullptr, host_pool_take(4096, &hp, nullptr, true));
        HIP_TRY(nullptr, hipHostGetDevicePointer(&dp, hp, 0));
        h->tot_host = static_cast<int32_t *>(hp);
        h->tot_dev = static_cast<int32_t *>(dp);
        std::memset(hp, 0, 64);
        return MPC_OK;
    }
};

}  // namespace
