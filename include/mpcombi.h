/*
 * mpcombi.h -- C ABI of the MI355X-native combinatorial mpLP/mpQP engine (libmpcombi_hip.so).
 *
 * The reference (PPOPT, pure Python) has no FFI; its plug points for this path are Python callables.
 * Each entry point below names the reference interface it replaces (paths relative to
 * /root/reference/src/ppopt):
 *
 *   mpc_create / mpc_destroy     the read-only `program` object every worker receives
 *                                (mpqp_program.py:29-42, mplp_program.py:60-134; matrices AFTER presolve)
 *   mpc_check_level              the batched operator  pool.map(lambda a: full_process(program, a, murder_list,
 *                                gen_children), to_check)   mp_solvers/mpqp_parrallel_combinatorial.py:110-116, :17-64
 *   mpc_frontier_* / mpc_level_* the same operator with the frontier (to_check), the pruned list (murder_list,
 *                                mp_solvers/solver_utils.py:15-55) and the children (future_list, driver :127-135) kept
 *                                resident in HBM between levels
 *   mpc_lp_solve_batch           the deterministic-solver plug  Solver.solve_lp(c, A, b, equality_constraints)
 *                                solver.py:211-246 -> solver_interface/cvxopt_interface.py:153-208, batched
 *
 * Conventions: plain pointers and sizes, row-major float64, int32 indices, caller-owned buffers that are
 * copied at creation; integer return codes (0 = MPC_OK), never C++ exceptions; per-candidate numerical
 * trouble is a status value, not an error.  A handle is bound to one device and one stream and is not
 * re-entrant; use one handle per GPU.  Calls that read or write caller-owned memory (host or device pointers) have
 * completed on the handle's stream when they return; device pointers handed in must be ready (the caller synchronises
 * its own stream first).
 */
#ifndef MPCOMBI_H
#define MPCOMBI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_OK 0
#define MPC_ERR_INVALID 1      /* bad argument / unsupported dimensions                      */
#define MPC_ERR_HIP 2          /* a HIP runtime call failed (mpc_last_error has the text)     */
#define MPC_ERR_CAPACITY 3     /* caller buffer too small; required size returned in-place    */
#define MPC_ERR_STATE 4        /* call sequence error (e.g. level results requested before run) */

/* per-candidate status == verdict of full_process (driver lines 17-64) */
#define MPC_INFEASIBLE 0        /* rank deficient (numpy's SVD rule, constraint_utilities.py:222-236) or (x,theta) LP infeasible -> pruned */
#define MPC_FEASIBLE 1          /* feasible, not optimal -> children.  "Not optimal" is the reference's: its optimality LP maximises t
                                   (mpqp_program.py:203-322) and anything but an optimal status is None -- also an UNBOUNDED t on a
                                   parameter set that is open in some direction (k_recession poses that question for such programs) */
#define MPC_OPTIMAL_NO_REGION 2 /* optimal, region lower dimensional (gen_cr returned None) -> pruned      */
#define MPC_REGION 3            /* critical region -> children                                             */
#define MPC_SINGULAR_KKT 4      /* feasible, KKT matrix numerically singular: no region, children expanded */
#define MPC_LP_LIMIT 5          /* an LP hit its iteration limit: treated as MPC_FEASIBLE by the driver    */

/* LP status of mpc_lp_solve_batch (anything but OPTIMAL is `None` in the reference) */
#define MPC_LP_OPTIMAL 0
#define MPC_LP_INFEASIBLE 1
#define MPC_LP_UNBOUNDED 2
#define MPC_LP_ITERLIMIT 3

#define MPC_MASK_WORDS 2        /* active sets as bit masks of 64-bit words: 2 words for n_c <= 128, 4 for n_c <= 256 (mpc_mask_words) */
#define MPC_MAX_NC 256
#define MPC_MAX_ROWS 192        /* n_c + n_tc + 1 */

typedef struct mpc_handle mpc_handle;

/* A presolved multiparametric program:  min 1/2 x'Qx + theta'H'x + c'x  s.t.  A x <= b + F theta
 * (first n_eq rows are equalities),  A_t theta <= b_t.   Q == NULL => mpLP. */
typedef struct {
    int32_t n_x, n_t, n_c, n_eq, n_tc;
    const double *A;   /* n_c  x n_x */
    const double *b;   /* n_c        */
    const double *F;   /* n_c  x n_t */
    const double *c;   /* n_x        */
    const double *H;   /* n_x  x n_t */
    const double *Q;   /* n_x  x n_x, or NULL */
    const double *A_t; /* n_tc x n_t */
    const double *b_t; /* n_tc       */
} mpc_problem;

typedef struct {
    int64_t n;             /* candidates in the level                                 */
    int32_t k;             /* their cardinality (incl. equalities)                    */
    int32_t kkt_mode;      /* 0 Schur/Cholesky (Q > 0), 1 dense KKT LU (mpLP, PSD Q)    */
    int64_t n_status[6];   /* histogram of the status byte                            */
    int64_t n_regions;     /* == n_status[MPC_REGION]                                 */
    int64_t n_children;    /* size of the next frontier (0 when gen_children == 0)    */
    int64_t n_pruned_new;  /* masks appended to the pruned list by this level         */
    int64_t lp_pivots;     /* simplex pivots executed by this level (all LPs)         */
    float ms_verdict, ms_region, ms_children, ms_total; /* HIP-event times on the handle's stream */
    int64_t n_xtheta_lp;   /* candidates whose feasibility needed the large (x,theta) LP */
    int64_t n_xtheta_fallback; /* ... of which the vertex warm start was abandoned for a from-scratch solve */
    int64_t wave_cycles[4];    /* wavefront cycles in: KKT solve, theta LP, (x,theta) LP, region build */
    int64_t n_region_retry;    /* optimal candidates re-solved by the LDS-engine region kernel */
    int64_t n_x_cached;        /* (x,theta) solves that started from the parent's dictionary cached in HBM */
    /* HIP-event time of single launches of this level (0 when the kernel did not run): k_theta2, the main k_x2 launch
     * (over n_x_items candidates), k_region2 (over n_opt candidates); region_side_stream = 1: that k_region2 launch ran on the
     * handle's side stream UNDER the (x,theta) stage (its time is not on the level's critical path), 0: in line; mpc_solve_start's
     * loop also reports 2: the launch of this small level ran beside the level AFTER it (the level was published one level later),
     * 3: such a launch missed (mpc_set_region_overlap) and these are the figures of the level's repeat in line */
    float ms_theta, ms_x, ms_region2, region_side_stream;
    int64_t n_x_items, n_opt;
    int64_t dict_read_bytes;   /* bytes of one cached dictionary record as k_x2 reads it (0: no cache on this level)   */
    int64_t dict_write_bytes;  /* bytes of one record as k_x2 stores it for the next level (0: nothing stored)         */
    int64_t n_theta_items;     /* candidates k_theta2 processed (those the thread kernel's screen left open)             */
    int64_t n_region_rows;     /* rows [f | E] the region kernel appended to the row pool (streamed levels: rows of erows in use) */
    /* HIP-event times of k_kkt_thread (over n candidates) and of the last level's quick test k_xq / k_xq_grouped (over n_xq_items
     * candidates, xq_pivots product-form iterations: each reads one column and one row of the parent's record) */
    float ms_kkt, ms_xq;
    int64_t n_xq_items, xq_pivots;
    int64_t xq_record_ints, xq_record_rows, xq_record_cols;   /* 2 mr + NXC + 3 ints, mr rows, n_d0c + 1 columns of a record */
    /* round 5: the quick test's first pass with one thread per candidate (k_xq_thread): candidates it decided (of n_xq_items; the
     * wavefront kernel gets the others) and its HIP-event time (inside ms_xq) */
    int64_t n_xq_thread;
    float ms_xq_thread, xq_thread_beside_theta;   /* 1: the pass ran on the second stream beside the theta stage (outside ms_xq), 0: inside ms_xq */
    /* round 5: one-step plans on a level that keeps dictionaries: records written by k_x1 (the streamed single pivot), its HIP-event
     * time and that of the plan pass (k_xq_thread in plan mode) -- both inside ms_x, whose remainder is the register simplex k_x2 */
    int64_t n_x1;
    float ms_x1, ms_x_plan;
} mpc_level_stats;

/* ---- library / device ------------------------------------------------------------------------------ */
int mpc_device_count(void);
const char *mpc_version(void);
/* text of the last error of a call that had no handle (mpc_create, mpc_lp_solve_batch) */
const char *mpc_last_global_error(void);

/* ---- program handle ---------------------------------------------------------------------------------- */
/* stream: a hipStream_t (as void*) the handle should launch on, or NULL to create its own. */
int mpc_create(const mpc_problem *problem, int32_t device, void *stream, mpc_handle **out);
int mpc_destroy(mpc_handle *h);
const char *mpc_last_error(const mpc_handle *h);
/* fixed strides of one region record for this program (see mpc_level_regions) */
int64_t mpc_region_doubles(const mpc_handle *h);
int64_t mpc_region_ints(const mpc_handle *h);
/* dynamic LDS bytes per wavefront of the verdict / region kernels (for reports) */
int32_t mpc_lds_bytes(const mpc_handle *h, int32_t which);
/* The one-off dense blocks of the program as the device holds them (diagnostics, tests).  For a positive definite Q they are
 * formed at mpc_create by the MFMA set-up kernel (csrc/setup_mfma.hip: blocked Cholesky of Q and the products below as
 * v_mfma_f64_16x16x4_f64 tiles) and replace the per-active-set dense KKT factorisation of MPQP_Program.optimal_control_law
 * (mpqp_program.py:182-198):  which = 0: W = A Q^-1 A' (n_c x n_c), 1: UV = [A Q^-1 c + b | A Q^-1 H + F] (n_c x (n_t+1)),
 * 2: Gt = A Q^-1 (n_c x n_x), 3: X0H = -Q^-1 [c | H] (n_x x (n_t+1)), 4: A A' (n_c x n_c; any program).  *n = number of doubles
 * (0 for which < 4 when Q is absent or not positive definite); MPC_ERR_CAPACITY when cap < *n.
 * which = 5..10: the blocks with the program's n_eq equality rows E (members of every active set) eliminated, so that the Schur
 * system of an active set E + a is the one of `a` alone:  5: Wr = W - W[:,E] W_EE^-1 W[E,:], 6: UVr = UV - W[:,E] W_EE^-1 UV[E,:],
 * 7: (A A')r likewise, 8: Me = W_EE^-1 UV[E,:] (n_eq x (n_t+1)), 9: Ne = W_EE^-1 W[E,:] (n_eq x n_c), 10: the n_eq pivots of the
 * Gram elimination of E, then the n_eq diagonal entries of A_E A_E'.  *n = 0 when n_eq = 0 or the elimination is not in use. */
int mpc_program_block(mpc_handle *h, int32_t which, double *out_host, int64_t cap, int64_t *n);
/* the HIP stream the handle launches on (hipStream_t as void*) */
void *mpc_stream(const mpc_handle *h);

/* ---- frontier (to_check) and pruned list (murder_list), resident on the device ------------------------ */
/* generate_children_sets(equality_indices, n_c)  (driver line 98) */
int mpc_frontier_root(mpc_handle *h);
int mpc_frontier_set(mpc_handle *h, const int32_t *cand_host, int64_t n, int32_t k);
int mpc_frontier_set_device(mpc_handle *h, const int32_t *cand_dev, int64_t n, int32_t k);
/* keep candidates rank, rank+world, ... of the resident frontier (multi-GPU: the ranks hold identical frontiers up to the
 * level at which they split; the kept candidates still find their parents' dictionaries in this GPU's cache) */
int mpc_frontier_shard(mpc_handle *h, int32_t rank, int32_t world);
int mpc_frontier_info(const mpc_handle *h, int64_t *n, int32_t *k);
int mpc_frontier_get(mpc_handle *h, int32_t *cand_host, int64_t cap);
int mpc_pruned_clear(mpc_handle *h);
int32_t mpc_mask_words(const mpc_handle *h);                                    /* words of one active-set mask for this program */
int mpc_pruned_add(mpc_handle *h, const uint64_t *masks_host, int64_t m);        /* m x mpc_mask_words(h) */
int mpc_pruned_add_device(mpc_handle *h, const uint64_t *masks_dev, int64_t m);
int64_t mpc_pruned_count(const mpc_handle *h);
int mpc_pruned_get(mpc_handle *h, uint64_t *masks_host, int64_t cap);

/* ---- one BFS level over the resident frontier --------------------------------------------------------- */
/* Runs verdict -> region -> (gen_children ? child generation against the CURRENT pruned list : nothing).
 * Sets pruned by this level become visible to child generation only after mpc_frontier_advance, which is the
 * reference's worker semantics (workers hold the murder_list of the previous levels, driver :110-131). */
int mpc_level_run(mpc_handle *h, int32_t gen_children, mpc_level_stats *stats);
int mpc_level_run_ex(mpc_handle *h, int32_t gen_children, int32_t flags, mpc_level_stats *stats);   /* flags: MPC_LEVEL_GRAPH, MPC_LEVEL_KEEP_LOWDIM */
int mpc_level_status(mpc_handle *h, uint8_t *status_host);                       /* n bytes, frontier order */
/* One level of SEVERAL programs per launch (reference: mp_solvers/mpmiqp_enumeration.py:41-50 maps solve_mpqp over the
 * binary fixations one sub-program at a time).  handles[0..n_handles) are distinct programs on one device, each with its own
 * resident frontier; gen_children[i] as in mpc_level_run; flags: MPC_LEVEL_KEEP_LOWDIM.  Every stage of the level is ONE launch for
 * all members (blockIdx.y = member, arguments from a table in device memory), the host synchronises once, and each member is left
 * in the state mpc_level_run would have left it -- same kernels' bodies, same lists: identical statuses, children and pruned masks,
 * and bit-identical region records except for the rare candidates that turn out optimal only after the theta stage (built here by
 * the register-resident region kernel with all others, by the LDS-engine kernel in the single-program form: same regions, coefficients
 * equal to ~1e-10, see csrc/batch_level.hpp); afterwards every handle is used on its own as usual (mpc_level_regions_slots, mpc_frontier_advance,
 * ...).  Members the batch form does not cover (no register-resident LP instantiation, MPC_NO_SMALLPATH=1, a level that needs the
 * LDS-engine region kernel or has a late optimal candidate) are run by mpc_level_run's own paths inside this call; *n_batched
 * (optional) = members that went through the shared launches.  stats (optional): n_handles entries. */
int mpc_level_run_batch(mpc_handle **handles, int32_t n_handles, const int32_t *gen_children, int32_t flags, mpc_level_stats *stats,
                        int32_t *n_batched);
/* For drivers that hold many handles: the device memory (GB) the next level of h's frontier will hold in a batch (what is charged
 * against MPC_BATCH_BUDGET_GB), and mpc_trim: an idle handle gives its level buffers (frontier, lists, region records, dictionary
 * cache, pruned list) back to the library's pool -- the program stays, a later solve allocates again. */
int mpc_frontier_advance_batch(mpc_handle **handles, int32_t n_handles);   /* mpc_frontier_advance for every handle of a list */
double mpc_level_memory_gb(const mpc_handle *h, int32_t gen_children);
int mpc_trim(mpc_handle *h);
/* The two halves of mpc_level_run_batch: _start queues the shared launches and returns (*token owns the state; the handles must not
 * be used until _wait), _wait synchronises, completes every member and runs the members outside the shared launches.  A token is
 * consumed by exactly one _wait. */
int mpc_level_batch_start(mpc_handle **handles, int32_t n_handles, const int32_t *gen_children, int32_t flags, void **token);
int mpc_level_batch_wait(void *token, mpc_level_stats *stats, int32_t *n_batched);
/* The same level driven by the handle's worker thread: mpc_level_start returns at once, mpc_level_wait joins it and returns
 * what mpc_level_run would have returned.  Between the two only mpc_level_stream_info / mpc_level_chunk_wait may be called
 * on the handle.  (Reference: the parent process is free while pool.map runs, driver :116, and merges results as they come.)
 * flags & MPC_LEVEL_STREAM: the region records of the level are STREAMED to the host while the region kernel runs -- the
 * kernel writes head_d / head_i / erows (layout of mpc_level_regions_slots, one slot per optimal candidate) straight into
 * page-locked host memory and raises one flag per chunk of slots, so the caller builds its region objects chunk by chunk
 * under the kernel instead of fetching everything afterwards.
 *   mpc_level_stream_info  blocks until the region stage of the running level has been launched; hands over the three
 *                          arrays (the CALLER owns them from then on: mpc_host_free), the number of slots, the row
 *                          capacity of erows, the chunk size (slots) and the number of chunks.  n_slots == 0: this level
 *                          does not stream (no optimal candidate, a shape outside the register-engine region kernel, or
 *                          more than 1 GiB of records) -- fetch with mpc_level_regions_slots after mpc_level_wait.
 *   mpc_level_chunk_wait   blocks until every slot of chunk j (slots j*chunk .. ) is complete in host memory.  head_d and
 *                          erows of a chunk are complete with its flag as well.
 *   mpc_level_stream_fixup after mpc_level_wait, when stats.n_region_retry > 0: fills the slots of the candidates that were
 *                          re-solved by the LDS-engine kernel (their head_i[0] was MPC_STREAM_RETRY while streaming); rows
 *                          are appended behind stats.n_region_rows, *n_rows = rows in use afterwards. */
#define MPC_LEVEL_STREAM 1
/* MPC_LEVEL_THEN_BASE (mpc_level_start, with gen_children == 0): behind this -- the last -- level the worker also checks the
 * base active set, the equality rows alone (driver :142-146), while the caller still consumes the level's streamed records;
 * mpc_base_result returns its status and fixed-stride region record (layout of mpc_level_regions) once, MPC_ERR_STATE when
 * the check did not run (the caller then uses mpc_check_level).  Frontier, level results and the pruned list of the handle
 * then belong to the base set. */
#define MPC_LEVEL_THEN_BASE 8
/* MPC_LEVEL_GRAPH (gen_children must be 0): the question of the connected-graph traversals (mp_solvers/mpqp_combi_graph.py:
 * 48-66, feasability_check) instead of full_process -- rank test, KKT solve, "is the critical region non-empty" (the theta
 * LP over multiplier, slack and A_t rows), region.  The (x,theta) feasibility LP is not posed.  Statuses: MPC_INFEASIBLE =
 * rank deficient, MPC_FEASIBLE = full rank, empty region, MPC_OPTIMAL_NO_REGION = non-empty but lower dimensional,
 * MPC_REGION.  Nothing is appended to the pruned list. */
#define MPC_LEVEL_GRAPH 4
/* MPC_LEVEL_KEEP_LOWDIM: the rule of the SERIAL driver (mp_solvers/mpqp_combinatorial.py:44-61) and of the _exp parallel driver
 * (mpqp_parallel_combinatorial_exp.py:38-52): a set that is optimal with a lower-dimensional region is expanded like any
 * feasible set and is not put on the pruned list.  Without the flag the parallel driver's rule applies (:57-59): such a set is
 * pruned together with its supersets, which can lose regions on degenerate programs. */
#define MPC_LEVEL_KEEP_LOWDIM 16
/* MPC_LEVEL_ONLY_BASE (mpc_level_start): the worker checks the base active set ONLY -- no level is run, the frontier is replaced by
   the base set; result through mpc_base_result after mpc_level_wait.  For a second handle of the same program (`twin`): the
   driver starts the check there when the solve reaches its first large level, and the check's chain of small kernels (0.45 ms
   at config 4) runs under the large levels of the main handle instead of behind the last one. */
#define MPC_LEVEL_ONLY_BASE 32
#define MPC_STREAM_RETRY 7
/* Whether the region stage of a level may be launched under its (x,theta) stage (default 1; environment MPC_NO_ROVERLAP=1 = 0).
 * An overlapped launch reserves spare record slots for candidates that turn out optimal only after it (re-solved doubtful ones);
 * should a level ever find more of them than it reserved, mpc_level_run / mpc_level_wait return MPC_ERR_CAPACITY -- no
 * candidate is demoted -- and the caller repeats the solve with on = 0, where every optimal candidate is known at launch.
 * (Reference: full_process never loses a region, mp_solvers/mpqp_parrallel_combinatorial.py:52-61.)
 * The same switch governs the other overlap of a region stage: inside mpc_solve_start's loop the region stage of a SMALL level runs beside
 * the kernels of the level after it (its children are generated before its regions exist; a region that turns out lower-dimensional
 * abandons the pass once and switches this off for the handle).  on = 0: neither overlap; 1 (default): both; 2: large levels as with 1,
 * small levels build their regions in line (A/B, tests); 3 (tests): as 1, and the first small level closed that way on this handle
 * reports a miss. */
int mpc_set_region_overlap(mpc_handle *h, int32_t on);
/* mpc_set_timing(h, 0): the levels of this handle run WITHOUT the HIP-event records around their stages and heavy kernels -- about
 * fourteen records per large level, four per small one, each a marker the queue stops at (measured, one MI355X: 0.16 ms of a 4.9 ms
 * config-4 solve, 0.11 of a 1.1 ms config-2 solve).  The ms_* fields of mpc_level_stats are then 0, every count is as before.  The host
 * layer switches the records on for the solves that ask for a profile.  Default: on (MPC_NO_KEV=1 in the environment: off). */
int mpc_set_timing(mpc_handle *h, int32_t on);
/* mpc_engine_kind: which kernels this handle's levels run on (diagnostics: the shape sweep records it per cell).  out[0] = 1 the
 * register-resident kernels (k_kkt_thread / k_theta2 / k_x2 / k_region2 ...), 0 the LDS-engine kernels (k_verdict / k_region);
 * out[1] = rows per lane of the theta LP (1 / 2; 0: none), out[2] = of the (x,theta) dictionary, out[3] = of the region LP (0: the
 * LDS-engine region kernel); out[4] = compile-time n_theta of the instantiation (4 / 8 / 10); out[5] = 1: the parameter set is open in
 * some direction (k_recession behind the verdict stages); out[6] = KKT mode (0 Schur / Cholesky, 1 dense); out[7] = largest number of
 * inequality rows k_kkt_thread solves for.  (No counterpart in the reference: it has one code path for every program,
 * mplp_program.py:411-444.) */
int mpc_engine_kind(mpc_handle *h, int32_t out[8]);
int mpc_level_start(mpc_handle *h, int32_t gen_children, int32_t flags);
int mpc_level_stream_info(mpc_handle *h, double **head_d, int32_t **head_i, double **erows, int64_t *n_slots, int64_t *cap_rows,
                          int32_t *chunk, int32_t *n_chunks);
int mpc_level_chunk_wait(mpc_handle *h, int32_t j);
int mpc_level_wait(mpc_handle *h, mpc_level_stats *stats);
int mpc_level_stream_fixup(mpc_handle *h, double *head_d, int32_t *head_i, double *erows, int64_t *n_rows);
int mpc_base_result(mpc_handle *h, uint8_t *status, int64_t *n_regions, double *rec_d, int32_t *rec_i);
/* The WHOLE level loop of the reference's driver behind one call (mp_solvers/mpqp_parrallel_combinatorial.py:98-139: root frontier =
 * children of the equality set, then per level pool.map(full_process) -> merge pruned / children / regions -> next level), run by
 * the handle's worker thread: no level is handed back to the caller, so the device never waits for the host between levels
 * (round 3: 0.38 ms of a 6.7 ms solve of config 4 sat in those hand-overs, tools/gpu_idle.sh).  The caller only CONSUMES: per level
 * it receives the region records while later levels already run.
 *   mpc_solve_start(h, max_levels, flags)  clears the pruned list, roots the frontier and starts the loop for at most max_levels
 *          levels (the last one without children, driver :108).  flags: MPC_LEVEL_STREAM (large levels stream their records),
 *          MPC_LEVEL_KEEP_LOWDIM, MPC_SOLVE_FETCH (records of levels that do not stream are copied to page-locked host arrays by the
 *          loop), MPC_LEVEL_THEN_BASE (the base active set is checked behind the last level: mpc_base_result).
 *   mpc_solve_level(h, level, &info)       blocks until level `level` (0-based) has records to hand over or has finished.
 *          info.mode: 1 = streamed (arrays are being written; chunk j readable after mpc_solve_chunk_wait(h, level, j); layout of
 *          mpc_level_stream_info), 2 = complete arrays (n_slots slots, n_rows rows in use), 0 = the level has no records,
 *          -1 = the loop ended before this level (return code = the loop's).  Arrays are the caller's from then on (mpc_host_free).
 *   mpc_solve_level_wait(h, level, &stats, &ms_wall)  blocks until the level has finished: its statistics; when
 *          stats.n_region_retry > 0 the slots of the re-solved candidates of a streamed level have been filled in place (list the
 *          level's slots again: head_i[slot][0] == MPC_REGION).
 *   mpc_solve_wait(h, &n_levels)           joins the loop: its return code (MPC_ERR_CAPACITY as for mpc_level_wait) and the number
 *          of levels completed.  The handle is then in the state after the last level (mpc_frontier_info, mpc_level_* fetches). */
#define MPC_SOLVE_FETCH 64
typedef struct {
    int32_t level, k;          /* 0-based level, cardinality of its candidates                                   */
    int32_t mode;              /* see above                                                                      */
    int32_t chunk, n_chunks;   /* mode 1: slots per chunk, number of chunks                                      */
    int32_t pad_;
    int64_t n;                 /* candidates of the level                                                        */
    int64_t n_slots;           /* rows of head_d / head_i                                                        */
    int64_t n_rows;            /* mode 1: row capacity of erows; mode 2: rows in use                             */
    double *head_d;            /* [n_slots][fd]     fd = n_x n_t + n_x + k n_t + k                               */
    int32_t *head_i;           /* [n_slots][fi]     fi = 8 + k + n_tc + k + 2 (n_c - k)                          */
    double *erows;             /* [n_rows][n_t + 1] */
} mpc_solve_level_info;
int mpc_solve_start(mpc_handle *h, int32_t max_levels, int32_t flags);
int mpc_solve_level(mpc_handle *h, int32_t level, mpc_solve_level_info *info);
int mpc_solve_chunk_wait(mpc_handle *h, int32_t level, int32_t j);
int mpc_solve_level_wait(mpc_handle *h, int32_t level, mpc_level_stats *stats, double *ms_wall);
int mpc_solve_wait(mpc_handle *h, int32_t *n_levels);
/* Region records of this level in frontier order.  cand_index[i] = position of region i's candidate.
 *   rec_d (mpc_region_doubles each): A_x[n_x*n_t] b_x[n_x] A_l[n_c*n_t] b_l[n_c] E[(n_c+n_tc)*n_t] f[n_c+n_tc]
 *   rec_i (mpc_region_ints each):    k n_E n_omega n_lambda n_regular | active[n_c] | omega[n_tc] | lambda[n_c]
 *                                     | regular_idx[n_c] | regular_con[n_c]                      (unused = -1)
 * i.e. every field of CriticalRegion (critical_region.py:34-48); E/f are the non-redundant unit-norm rows
 * before exact-duplicate removal. */
int mpc_level_regions(mpc_handle *h, double *rec_d_host, int32_t *rec_i_host, int64_t *cand_index_host, int64_t cap);
/* The same regions in compact form (what the device writes; no padding to n_c):
 *   head_d (fd doubles each): A_x[n_x*n_t] b_x[n_x] A_l[k*n_t] b_l[k]
 *   head_i (fi ints each):    3 cand nE n_omega n_lambda n_regular e_off 0 | active[k] | omega[n_tc] | lambda[k]
 *                             | regular_idx[n_c-k] | regular_con[n_c-k]            (unused = -1)
 *   erows  (n_t+1 doubles each): f, E[0..n_t)  -- region i owns rows e_off .. e_off+nE-1
 * mpc_compact_strides gives fd, fi for the current frontier (they depend on its cardinality k) and an upper bound
 * of the number of rows this level's regions own. */
int mpc_compact_strides(const mpc_handle *h, int64_t *fd, int64_t *fi, int64_t *max_rows);
int mpc_level_regions_compact(mpc_handle *h, double *head_d, int32_t *head_i, int64_t cap_regions, double *erows,
                              int64_t cap_rows, int64_t *n_regions, int64_t *n_rows);
/* The same data without any host-side repacking: ALL slots the region kernel wrote (one per optimal candidate, frontier
 * order), copied straight into the caller's arrays.  head_i[slot][0] is the candidate's final status: only slots with
 * MPC_REGION are regions (the others were optimal but lower dimensional); rows are referenced through e_off and are
 * not in slot order.  n_slots <= cap_slots = mpc_level_slots(h); cap_rows from mpc_compact_strides.  With arrays from
 * mpc_host_alloc the copies are direct DMA transfers. */
int64_t mpc_level_slots(const mpc_handle *h);
int mpc_level_regions_slots(mpc_handle *h, double *head_d, int32_t *head_i, int64_t cap_slots, double *erows,
                            int64_t cap_rows, int64_t *n_slots, int64_t *n_rows);
/* mpc_level_regions_slots that returns as soon as head_i has arrived: head_d and erows (the large arrays) are still
 * being written by DMA on the handle's stream when it returns and are complete after the next call that synchronises
 * the handle -- mpc_sync, or any mpc_level_run.  The arrays must be page-locked (mpc_host_alloc) and must stay alive until
 * then.  When some record needs host-side repacking the call behaves like mpc_level_regions_slots. */
int mpc_level_regions_slots_async(mpc_handle *h, double *head_d, int32_t *head_i, int64_t cap_slots, double *erows,
                                  int64_t cap_rows, int64_t *n_slots, int64_t *n_rows);
/* The same, not even waiting for head_i: all three arrays are complete after mpc_sync or the next level of the handle
 * (mpc_level_run, mpc_level_batch_start) -- the driver of a batch queues the fetches of every member, starts the next level for all of
 * them and builds the region objects of the finished level while the device works. */
int mpc_level_regions_slots_nowait(mpc_handle *h, double *head_d, int32_t *head_i, int64_t cap_slots, double *erows,
                                   int64_t cap_rows, int64_t *n_slots, int64_t *n_rows);
/* mpc_level_regions_slots_nowait for every handle of a list in one call (the driver of a batch: one call per level instead of one
 * per member).  Arrays of n_handles entries; a member without regions gets n_slots = n_rows = 0 and may pass null buffers. */
int mpc_level_batch_fetch(mpc_handle **handles, int32_t n_handles, double *const *head_d, int32_t *const *head_i, const int64_t *cap_slots,
                          double *const *erows, const int64_t *cap_rows, int64_t *n_slots, int64_t *n_rows);
int mpc_sync(mpc_handle *h);   /* waits for everything queued on the handle's stream (and for a pending shared record copy of mpc_level_batch_fetch) */
/* mpc_level_batch_fetch copies the records of all members that hold them in slot form with ONE launch (round 5); mpc_fetch_wait waits
 * for that launch on the given device (mpc_sync of any member and the next mpc_level_batch_start do so too) */
int mpc_fetch_wait(int32_t device);
/* ---- the level loop of MANY programs inside the library (round 5) -------------------------------------------------------------------
 * The caller of the combinatorial path for many small programs -- the mixed-integer enumeration maps solve_mpqp over its sub-programs
 * (reference mp_solvers/mpmiqp_enumeration.py:41-50), each of which runs the level loop of mpqp_parrallel_combinatorial.py:102-139 -- as
 * ONE loop on a thread of the library: shared launches of a level for all members (mpc_level_batch_start / _wait), the record copy of
 * the level for all members into three page-locked blocks (mpc_level_batch_fetch), the members' frontier hand-overs, the next level.
 * The device never waits for the caller between levels; the caller only consumes, level by level:
 *   mpc_solve_many_start(handles, n, max_levels[n], flags, &job)   every handle: pruned list cleared, frontier rooted, then the loop
 *          (flags: MPC_LEVEL_KEEP_LOWDIM).  The handles must not be touched until mpc_solve_many_wait has returned.
 *   mpc_solve_many_level(job, level, &info)   blocks until level `level` (0-based) has been run and its records are COMPLETE in the
 *          three blocks (member j's arrays start at off_d[j] / off_i[j] / off_e[j] elements, n_slots[j] slots of the member's fd / fi,
 *          n_rows[j] rows of n_t + 1).  The blocks are the caller's from then on (mpc_host_free; null when no member found a region);
 *          the small arrays of `info` live until mpc_solve_many_wait.  info.n_members == 0: the loop ended before this level --
 *          info.done = 1: every member has run its last level; 2: the next level of the remaining members does not fit the memory budget
 *          of the shared launches together (MPC_BATCH_BUDGET_GB): their frontiers are advanced, their next level has NOT been started,
 *          the caller takes over (admission / parking: the host layer's loop).
 *   mpc_solve_many_wait(job)   joins the loop and frees the job: the loop's return code (the failing member carries the message).
 * flags & MPC_SOLVE_MANY_BASE: when every member has run its last level (not after a hand-over) the loop closes with one more shared level
 * over the BASE active set of every program (the equality rows alone, one candidate each, pruned lists cleared: the reference tests it
 * last, mpqp_parrallel_combinatorial.py:142-146); that level's info carries base = 1. */
#define MPC_SOLVE_MANY_BASE 128
typedef struct {
    int32_t level, n_members, n_shared, done;
    int32_t base, pad_;              /* base = 1: this is the closing level of the base active sets (MPC_SOLVE_MANY_BASE)   */
    const int32_t *member;           /* [n_members] positions in the handle array of mpc_solve_many_start          */
    const mpc_level_stats *stats;    /* [n_members]                                                                 */
    const int64_t *n_slots, *n_rows; /* [n_members] record slots / region rows copied (0: the member found no region) */
    const int64_t *off_d, *off_i, *off_e;   /* [n_members] element offsets inside head_d / head_i / erows            */
    double *head_d;
    int32_t *head_i;
    double *erows;
    int64_t len_d, len_i, len_e;     /* elements of the three blocks                                                */
    double ms_wall;                  /* wall time of the level on the loop's thread                                 */
} mpc_many_level_info;
int mpc_solve_many_start(mpc_handle **handles, int32_t n_handles, const int32_t *max_levels, int32_t flags, void **job);
int mpc_solve_many_level(void *job, int32_t level, mpc_many_level_info *info);
int mpc_solve_many_wait(void *job);
/* Page-locked host memory from a recycling pool (blocks return to the pool on mpc_host_free and are handed out again
 * without re-pinning).  For result arrays that are filled by mpc_level_regions_slots. */
int mpc_host_alloc(uint64_t bytes, void **out);
int mpc_host_free(void *p);
int mpc_level_children(mpc_handle *h, int32_t *children_host, int64_t cap);     /* n_children x (k+1) */
int mpc_level_children_device(mpc_handle *h, int32_t *children_dev, int64_t cap);
int mpc_level_pruned_new(mpc_handle *h, uint64_t *masks_host, int64_t cap);
/* The slot arrays of mpc_level_regions_slots copied device -> device into caller-owned DEVICE buffers (the multi-GPU
 * driver all-gathers them over RCCL without a host round trip; reference: the parent's merge of the workers' regions,
 * mpqp_parrallel_combinatorial.py:127-131).  cap_slots >= mpc_level_slots(h), cap_rows from mpc_compact_strides.
 * MPC_ERR_STATE when some record of the level is not in slot form on the device (regions re-solved by the LDS-engine
 * kernel): the caller then uses mpc_level_regions_slots. */
int mpc_level_regions_device(mpc_handle *h, double *head_d_dev, int32_t *head_i_dev, double *erows_dev, int64_t cap_slots,
                             int64_t cap_rows, int64_t *n_slots, int64_t *n_rows);
int mpc_level_pruned_new_device(mpc_handle *h, uint64_t *masks_dev, int64_t cap);
/* frontier := children of this level; pruned list += sets pruned by this level  (driver :127-135) */
int mpc_frontier_advance(mpc_handle *h);

/* ---- connected-graph traversals with the bookkeeping on the device ----------------------------------------------------- */
/* Reference: mp_solvers/mpqp_combi_graph.py:68-145 (variant 0: sets S / E, explore_subset / explore_superset around every
 * active set whose critical region is non-empty) and mp_solvers/mpqp_graph.py:38-108 (variant 1: attempted, generate_reduce,
 * generate_extra through the facet constraints of every full-dimensional region).  The traversal advances a whole WAVE of
 * active sets at a time; the wave, the set of everything ever queued and the neighbours emitted by the wave stay in HBM as
 * sorted arrays of masks (mpc_mask_words words each), so the order of the regions is deterministic.
 *   mpc_graph_begin       seeds (host masks, duplicates allowed) -> first wave
 *   mpc_graph_wave        the groups of the current wave, one (or, beyond 4M masks, several) per cardinality; n_groups == 0:
 *                         the traversal is complete
 *   mpc_graph_group_run   one group = one frontier of the level kernels (MPC_LEVEL_GRAPH verdicts: neither traversal needs the
 *                         (x,theta) feasibility LP -- without a pruning list "infeasible" and "not optimal" hand on the same
 *                         neighbours); afterwards mpc_level_status / mpc_level_regions_slots etc. describe that group; the
 *                         group's neighbours are appended to the pending list
 *   mpc_graph_wave_close  pending -> sorted, deduplicated, minus everything queued before = the next wave */
int mpc_graph_begin(mpc_handle *h, const uint64_t *seed_masks_host, int64_t n_seeds, int32_t variant);
int mpc_graph_wave(mpc_handle *h, int32_t *k_list, int64_t *count_list, int32_t cap, int32_t *n_groups, int64_t *n_wave, int64_t *n_visited);
int mpc_graph_group_run(mpc_handle *h, int32_t group, mpc_level_stats *stats);
int mpc_graph_wave_close(mpc_handle *h, int64_t *n_next, int64_t *n_visited);

/* ---- the batched operator with host buffers (drop-in for pool.map(full_process)) ---------------------- */
/* Uploads cand (n x k) and the pruned masks (m x mpc_mask_words(h); replaces the handle's list), runs the level
 * and downloads status, regions and children.  On MPC_ERR_CAPACITY *n_regions / *n_children hold the
 * required capacities. */
int mpc_check_level(mpc_handle *h, const int32_t *cand, int64_t n, int32_t k, const uint64_t *pruned_masks, int64_t m,
                    int32_t gen_children, uint8_t *status, int64_t *n_regions, double *rec_d, int32_t *rec_i,
                    int64_t *region_cand, int64_t region_cap, int64_t *n_children, int32_t *children,
                    int64_t children_cap);

/* ---- deterministic-solver plug: a batch of small dense LPs, one wavefront each ------------------------- */
/* min c'x s.t. A x <= b (rows flagged in eq as equalities), x free.  A: n_lp x m x n unless shared_A != 0
 * (then m x n, likewise b with shared_b, c with shared_c; c may be NULL = feasibility); eq: n_lp x m bytes.
 * Outputs (host): status[n_lp]; x[n_lp x n] and obj[n_lp] may be NULL. */
int mpc_lp_solve_batch(int32_t device, int64_t n_lp, int32_t m, int32_t n, const double *A, int32_t shared_A,
                       const double *b, int32_t shared_b, const double *c, int32_t shared_c, const uint8_t *eq,
                       int32_t *status, double *x, double *obj, int32_t *iters);

/* ---- the QP of the program at fixed parameter points, batched: one wavefront per point --------------------------------- */
/* Replaces MPQP_Program.solve_theta (mpqp_program.py:109-143 -> Solver.solve_qp, quad_prog_interface.py:16-89) for programs
 * with positive definite Q:  min 1/2 x'Qx + (c + H theta)'x  s.t.  A x <= b + F theta, first n_eq rows as equalities.
 * theta m x n_t (host).  status[p]: 0 optimal, 1 infeasible at that point, 3 iteration limit.  x (m x n_x, NaN where not
 * optimal), lambda (m x n_c multipliers, >= 0 on inequality rows), active (m x n_c bytes: 1 = the constraint is tight) and
 * iters (complementary pivots) may be NULL.  The constants c_c + c_t'theta + 1/2 theta'Q_t theta are the caller's. */
int mpc_qp_solve_batch(mpc_handle *h, int64_t m, const double *theta_host, int32_t *status, double *x, double *lambda,
                       uint8_t *active, int32_t *iters);

/* ---- the mixed-integer QP at fixed parameter points, batched: one wavefront per (point, binary fixation) pair -------------- */
/* MPMIQP_Program.solve_theta / solve_theta_batch (reference: mpmiqp_program.py:55-69 -> Solver.solve_miqp) for a positive definite
 * continuous Hessian Q_c.  With the binaries y fixed to leaf l and z = [1; theta; y] (n_z = 1 + n_t + n_b), the continuous QP is
 * the LCP  s = UV z + W lambda  of mpc_qp_solve_batch with the same W = A_c Q_c^-1 A_c' for every pair; its minimiser is
 * x_c = X0 z - Gt' lambda and its objective, constants included, 1/2 x_c' Q_c x_c + (G z)' x_c + 1/2 z' K z.
 *   W n_c x n_c, UV n_c x n_z, X0 n_x_c x n_z, Gt n_c x n_x_c, Q_c n_x_c x n_x_c, G n_x_c x n_z, K n_z x n_z (n_x_c = n_x - n_b);
 *   the first n_eq of the n_c LCP rows are equalities; lcp_row[n_c]: the program row (of n_rows) each LCP row is.
 *   check n_check x n_z, check_eq[n_check]: rows decided on z alone -- a pair with  check z < -MPC_MIQP_CHECK_TOL  on an inequality
 *   or  |check z| > MPC_MIQP_CHECK_TOL  on an equality row is infeasible without a pivot.
 *   binary_index[n_b]: positions of the binaries among the n_x variables; Y n_leaves x n_b: the fixations; theta m x n_t.
 * Per point the lowest objective among the optimal pairs wins, the lowest leaf on ties.  Outputs (host): status[m] (0 optimal,
 * 1 infeasible at that point, 3 some pair hit the iteration limit), leaf[m] (-1 unless optimal), obj[m] (NaN unless optimal);
 * x (m x n_x: x_c with y spliced in, NaN unless optimal), lambda (m x n_rows, 0 on rows outside the LCP) and active (m x n_rows
 * bytes, tight LCP rows) may be NULL.  Device memory: 12 bytes per (point, leaf) pair; the caller bounds m. */
#define MPC_MIQP_CHECK_TOL 1e-9
int mpc_miqp_solve_batch(int32_t device, int32_t n_c, int32_t n_eq, int32_t n_x, int32_t n_t, int32_t n_b, const double *W,
                         const double *UV, const double *X0, const double *Gt, const double *Q_c, const double *G, const double *K,
                         int32_t n_check, const double *check, const uint8_t *check_eq, const int32_t *binary_index, int32_t n_rows,
                         const int32_t *lcp_row, int64_t n_leaves, const double *Y, int64_t m, const double *theta, int32_t *status,
                         int32_t *leaf, double *obj, double *x, double *lambda, uint8_t *active);

/* ---- Chebyshev centre and radius of every facet of a batch of polytopes, one wavefront per facet ------------------------- */
/* Replaces get_facet_centers (mp_solvers/solver_utils.py:204-250; one chebyshev_ball LP per facet, utils/chebyshev_ball.py:10-63)
 * of the geometric algorithm.  ef_rows: stacked rows [f | E] (n_t + 1 doubles each) of all polytopes, row_off[n_regions + 1];
 * facet q is row q.  Outputs per row: centre (n_t), radius, status (MPC_LP_*; centre and radius are 0 unless optimal). */
int mpc_facet_centres(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, double *centre,
                      double *radius, int32_t *status);

/* ---- hit-and-run sampling of a batch of polytopes -------------------------------------------------------------------- */
/* Hit-and-run chains in a batch of polytopes {x : A_p x <= b_p}; see DESIGN for the exact chain and its random stream.
 * ab_rows: stacked rows [b | A] (n + 1 doubles each) of all polytopes, row_off[n_poly + 1] (<= 256 rows per polytope, n <= 64);
 * start: one point per polytope; chain g = p * chains + k.  Emits a sample after every n_steps steps (samples * n_steps < 2^32).
 * status per chain: MPC_HR_OK, MPC_HR_OUTSIDE (the start violates a row), MPC_HR_UNBOUNDED (a chord without an end); a chain
 * whose status is not MPC_HR_OK has NaN samples.  ms: device time of the kernel (may be NULL). */
#define MPC_HR_OK 0
#define MPC_HR_OUTSIDE 1
#define MPC_HR_UNBOUNDED 2
int mpc_hit_and_run(int32_t device, int32_t n, int64_t n_poly, const int64_t *row_off, const double *ab_rows,
                    const double *start /* n_poly x n */, int64_t chains, int64_t samples, int64_t n_steps, uint64_t seed,
                    double *out /* n_poly x chains x samples x n, host */, int32_t *status /* n_poly x chains */, float *ms);

/* ---- 2-D and 1-D slices of a batch of polytopes (plots, exact coverage in a plane) ------------------------------------- */
/* The slice of every region {theta : E_r theta <= f_r} by the plane theta = theta0 + U z (U: n x 2 row-major, U[t][k]), clipped to the
 * box lo_k <= z_k <= hi_k (box = {lo0, lo1, hi0, hi1}, finite, lo < hi), as a convex polygon; see DESIGN for the method.
 * ef_rows: stacked rows [f | E] (n + 1 doubles each) of all regions, row_off[n_regions + 1] (<= 256 rows per region, 1 <= n <= 64).
 * Region r owns the vertex slots row_off[r] + 4 r .. row_off[r + 1] + 4 r + 3 (its rows + 4): vert holds count[r] vertices (z_0, z_1)
 * counter-clockwise from the vertex of smallest atan2 about their mean; edge_row[k] is the row whose edge starts at vertex k (the
 * region's own row index, or -1 .. -4 for the box sides z_0 <= hi0, z_1 <= hi1, z_0 >= lo0, z_1 >= lo1); area[r] the polygon's
 * area; slots past count[r] are not written.  status: MPC_SLICE_FULL, MPC_SLICE_EMPTY (count 0), MPC_SLICE_LOWDIM (a segment or a
 * point: area <= eps D^2, D the box diameter; the vertices found are given), ORed with MPC_SLICE_CUT when a box side is an edge.
 * eps (> 0, < 1) owns every tolerance: minimum edge length eps D, zero normal |E_i U| <= eps |E_i| max_k |U_k| (and parallel rows
 * |sin| <= eps), lower-dimensional area eps D^2.  ms: device time of the kernel (may be NULL). */
#define MPC_SLICE_FULL 0
#define MPC_SLICE_EMPTY 1
#define MPC_SLICE_LOWDIM 2
#define MPC_SLICE_CUT 4
int mpc_slice_polygons(int32_t device, int32_t n, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *theta0,
                       const double *U, const double *box, double eps, double *vert /* (row_off[n_regions] + 4 n_regions) x 2 */,
                       int32_t *edge_row /* row_off[n_regions] + 4 n_regions */, int32_t *count, double *area, int32_t *status, float *ms);
/* The slice of every region by the line theta = theta0 + u t within t_lo <= t <= t_hi (finite, t_lo < t_hi): interval[r] = [a, b]
 * (NaN for MPC_SLICE_EMPTY), status as above with MPC_SLICE_LOWDIM for b - a <= eps (t_hi - t_lo) and MPC_SLICE_CUT when an end is
 * t_lo or t_hi. */
int mpc_slice_intervals(int32_t device, int32_t n, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *theta0,
                        const double *u, double t_lo, double t_hi, double eps, double *interval /* n_regions x 2 */, int32_t *status,
                        float *ms);

/* ---- consumer of the path: point location over a solution's critical regions, batched ---------------------------- */
/* Replaces the loop of Solution.get_region / Solution.evaluate (solution.py:45-112, CriticalRegion.is_inside
 * critical_region.py:83-86) for many parameter points at once.
 *   row_off   n_regions + 1 offsets into ef_rows;  ef_rows  total_rows x (n_t+1): [f | E] of every region, stacked
 *   xlaw      n_regions x n_x x (n_t+1): [b | A] of every region
 *   Q, c, H   objective of the program (n_x x n_x, n_x, n_x x n_t; any may be NULL) -- only used with overlapping != 0
 * mpc_locator_query: theta m x n_t (host).  region[p] = index of the first region that contains the point (flags without
 * MPC_LOCATE_OVERLAPPING) or of the containing region with the lowest objective, ties to the later one (with it); -1 if
 * none.  "Contains" is all(E theta - f < tol), the strict test of CriticalRegion.is_inside (critical_region.py:83-86), or
 * with MPC_LOCATE_INCLUSIVE all(E theta <= f + tol): with tol = 0 the test `A @ theta <= b` of the reference's
 * PointLocation (upop/point_location.py:46,59), under which points on a facet belong to the region.
 * x (m x n_x, may be NULL) = A theta + b of that region, NaN where there is none. */
#define MPC_LOCATE_OVERLAPPING 1
#define MPC_LOCATE_INCLUSIVE 2
/* MPC_LOCATE_WALK: locate by walking through adjacent regions instead of scanning the list (needs
 * mpc_locator_set_adjacency; ignored with the two flags above).  A region that contains the point within tol, at a cost that
 * follows the length of the walk, not the number of regions; points the walk cannot resolve (no neighbour behind any violated
 * row, step limit) or cannot certify as the first match (two or more rows of the located region within 2 tol, or one whose
 * neighbour is unknown) are tested against every region in parallel.  Same result as the scan -- the FIRST such region of the
 * list -- provided the rows of neighbouring regions have comparable scale (unit rows) and no region reaches a corner with a
 * wedge angle under 60 degrees: there a point 2 tol inside the located region can lie within tol in an earlier one
 * (csrc/locate.hpp, loc_walk). */
#define MPC_LOCATE_WALK 4
typedef struct mpc_locator mpc_locator;
int mpc_locator_create(int32_t device, int32_t n_x, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows,
                       const double *xlaw, const double *Q, const double *c, const double *H, mpc_locator **out);
/* Facet adjacency of a complete, non-overlapping solution: masks n_regions x mask_words (active set of every region, all
 * different), row_info one int per stacked row = kind << 16 | id with kind 0: multiplier row of active constraint id (behind
 * it: the region without id), 1: row of inactive constraint id (behind it: the region with id added), 2: row of the
 * parameter set (behind it: nothing), 3: unknown. */
int mpc_locator_set_adjacency(mpc_locator *loc, int32_t mask_words, int32_t n_c, const uint64_t *masks, const int32_t *row_info);
int mpc_locator_query(mpc_locator *loc, int64_t m, const double *theta, double tol, int32_t flags, int64_t *region,
                      double *x, float *ms_locate);
/* The number of points that the last MPC_LOCATE_WALK / MPC_LOCATE_TREE query handed to the exhaustive pass (more than 16,384 of
 * a walk: the list scan; fewer: every (point, region) pair in parallel); 0 after a query that needed none. */
int mpc_locator_last_unresolved(mpc_locator *loc, int64_t *n_points);
int mpc_locator_destroy(mpc_locator *loc);

/* ---- point-location search trees over a solution's hyperplanes ------------------------------------------------- */
/* A binary tree over unit planes s(theta) = n.theta - o whose descent gives EXACTLY the scan's answer (the flags above, any query
 * tol_q <= the build tol).  Region j is classified through its expanded polytope P^_j = {E_i theta <= f_i + tol max(1, |E_i|)}: "+" if
 * min s over P^_j >= -band, "-" if max s <= band, in both children otherwise (also when both hold).  An internal node keeps
 * tau- = max over its "+"-only regions of max(0, -min s), tau+ = max over its "-"-only regions of max(0, max s), each widened by
 * 1e-9 (1 + |o| + |theta*|_1) (theta* the optimal point of the LP that gave it); a query visits the "+" child if s >= -tau- and the
 * "-" child if s <= tau+, and applies the scan's rule to the union of the visited leaves' lists (ascending region indices).
 *
 * mpc_tree_build: builds on the locator's device-resident rows and attaches the tree to the locator.
 *   planes      n_planes x (n_t + 1): unit [n | o] (|n| = 1 within 1e-6)
 *   cand_off, cand_plane  (may both be NULL) the planes of every region, CSR over regions (n_regions + 1 offsets): the split
 *               candidates of a node are the planes of its regions; NULL: every plane is a candidate
 *   tol         build tolerance (>= 0); band >= 0 (unit-normal distance); leaf_size >= 1; 1 <= max_depth <= 64
 *   budget      device bytes allowed for the classification bitsets (2 or 3 x n_regions x ceil(n_planes / 64) x 8); <= 0: 4 GiB
 * Limits (MPC_ERR_INVALID with a message, before any launch): n_t <= 16, <= 256 rows per region, the bitsets within the budget.
 * stats (may be NULL): shape, work and device milliseconds per stage. */
#define MPC_LOCATE_TREE 8   /* mpc_locator_query: descend the attached tree (MPC_ERR_INVALID without one or with tol > its tol) */
typedef struct mpc_tree_stats {
    int64_t n_nodes, n_leaves, depth, max_leaf, leaf_items;
    double mean_leaf;
    int64_t pairs, box_pairs, lps, pivots, capped, tau_lps;   /* classification pairs, decided by the box, LPs (both modes), pivots,
                                                                 LP runs stopped at the pivot cap (reported as unbounded), tau LPs */
    int64_t bitset_bytes;
    double ms_classify, ms_split, ms_tau, ms_total;            /* device time of k_tree_classify<0>, of the split / partition
                                                                 kernels, of k_tree_classify<1>; wall time of the whole build */
} mpc_tree_stats;
int mpc_tree_build(mpc_locator *loc, int32_t n_planes, const double *planes, const int64_t *cand_off, const int32_t *cand_plane, double tol,
                   double band, int32_t leaf_size, int32_t max_depth, int64_t budget, mpc_tree_stats *stats);
/* The attached tree: n_nodes nodes (node 0 the root; children have larger indices), n_items leaf entries. */
int mpc_locator_tree_size(mpc_locator *loc, int64_t *n_nodes, int64_t *n_items, int32_t *n_planes, double *tol);
/* node_plane[k] (-1: leaf), node_child[2k] ("+") / [2k + 1] ("-"), node_tau[2k] (tau-) / [2k + 1] (tau+), node_off[n_nodes + 1]: node
 * k's leaf list is items[node_off[k] .. node_off[k + 1]); planes n_planes x (n_t + 1) as built */
int mpc_locator_get_tree(mpc_locator *loc, double *planes, int32_t *node_plane, int32_t *node_child, double *node_tau, int64_t *node_off,
                         int32_t *items);
/* attaches a tree given as the arrays above (a tree built earlier, or read back); validated: indices in range, children after their
 * parent, tau >= 0, leaf lists ascending */
int mpc_locator_set_tree(mpc_locator *loc, int32_t n_planes, const double *planes, int64_t n_nodes, const int32_t *node_plane,
                         const int32_t *node_child, const double *node_tau, const int64_t *node_off, const int32_t *items, double tol);

/* ---- explicit controllers in closed loop (Solution.simulate) ------------------------------------------------------- */
/* mpc_locator_simulate: n trajectories of `steps` steps of theta+ = A theta + B u + c + w under the law u = x*(theta)[inputs] of the
 * locator's regions, in one launch (k_simulate, closed_loop.hpp).  Step k of trajectory p: a non-finite theta_k ends it (status 3);
 * j_k = the region mpc_locator_query returns for theta_k with the same tol and flags, and -1 ends it (status 2); u_k = the rows `inputs`
 * of j_k's law (x of mpc_locator_query, bit for bit); theta_{k+1,i} = c_i + sum_j A_ij theta_j + sum_l B_il u_l + w_i, each term rounded
 * on its own in this order (no fma; 0.0 start without c, no w term without a disturbance); |theta_{k+1} - theta_k|_inf <= stop_tol
 * (stop_tol >= 0) ends it after the step (status 1).  Status 0: all steps ran.  exit_step[p]: the index of the last state (steps for
 * status 0, k + 1 for status 1, k for 2 and 3).
 *   flags     MPC_LOCATE_OVERLAPPING / _INCLUSIVE as for mpc_locator_query; the locator: MPC_LOCATE_TREE (the attached tree, tol <= its
 *             tol), MPC_LOCATE_WALK (the adjacency walk from the previous region; needs adjacency, not with the two flags above), neither:
 *             the list scan; MPC_SIM_FINAL: record the final states only
 *   theta0    n x n_t;  A n_t x n_t, B n_t x n_u, c n_t (may be NULL), inputs n_u indices into the law's n_x rows (1 <= n_u <= 16)
 *   w         steps x n x n_t (step-major, may be NULL), or box_lo / box_hi (n_t each, may be NULL): w = lo + (hi - lo) U, U the 53-bit
 *             uniform of Philox4x32-10 under the key (seed mod 2^32, (seed >> 32) ^ MPC_SIM_KEY_SALT) at the counter (p mod 2^32, p >> 32,
 *             k, j): components 2j and 2j + 1 from words (0, 1) and (2, 3)
 *   budget    device bytes allowed (<= 0: 4 GiB)
 * Outputs, step-major: theta (steps + 1) x n x n_t (with MPC_SIM_FINAL: n x n_t, the state at exit_step), u steps x n x n_u, region
 * steps x n; after a trajectory's end theta and u are NaN (all bits set) and region -1.  status, exit_step n.
 * Limits (MPC_ERR_INVALID with a message, before any launch): n_t <= 16, 1 <= n_u <= 16, inputs in range, finite theta0, A, B, c, w
 * and box (lo <= hi), the budget.  stats (may be NULL). */
#define MPC_SIM_FINAL 16
#define MPC_SIM_KEY_SALT 0x636c6f6f
typedef struct mpc_sim_stats {
    int64_t traj_steps;   /* steps taken, over all trajectories (a step that ends a trajectory with status 2 counts) */
    int64_t crossings;    /* walk: regions crossed */
    int64_t fallbacks;    /* walk / tree: points settled by the lane's own list scan */
    int32_t mode;         /* the locator that ran: 0 the list scan, MPC_LOCATE_WALK, MPC_LOCATE_TREE */
    float ms;             /* device milliseconds of k_simulate */
} mpc_sim_stats;
int mpc_locator_simulate(mpc_locator *loc, int64_t n, int32_t steps, const double *theta0, int32_t n_u, const int32_t *inputs, const double *A,
                         const double *B, const double *c, const double *w, const double *box_lo, const double *box_hi, uint64_t seed,
                         double tol, double stop_tol, int32_t flags, int64_t budget, double *theta, double *u, int32_t *region, int32_t *status,
                         int32_t *exit_step, mpc_sim_stats *stats);

/* ---- vertex enumeration of a batch of polytopes (geometry.polytope_vertices, Solution.vertices) ------------------------ */
/* mpc_region_vertices: the vertices and rays of every polytope {theta : E theta <= f}, one workgroup each (k_region_vertices,
 * vertices.hpp: the double-description method on the homogenised cone {(theta, t) : f t - E theta >= 0, t >= 0}).
 *   ef_rows   [rows][n_t + 1] = [f | E], CSR over polytopes by row_off[n_poly + 1] (row_off[0] = 0): what the locator is built from
 *   tol       incidence: row r is tight at v when |f_r - e_r v| <= tol (1 + |f_r|); vertices within tol (1 + |v|_inf) of a vertex before
 *             them in lexicographic order are merged (counted in stats->merges)
 *   slab      generators per list of the first pass (<= 0: 256); a polytope whose list outgrows it is repeated with a 4x larger slab
 *             while that is <= max_slab (<= 0: 2^24) and one polytope's slab fits the budget; then it stays MPC_VX_OVERFLOW
 *   budget    device bytes of the slabs in flight (<= 0: 4 GiB)
 *   v_cap, r_cap  in: the rows of vertices / incidence and of rays; out: the rows needed.  MPC_ERR_CAPACITY when they do not fit
 *             (status, n_vert, n_ray and stats are filled, the arrays are not written).
 * Outputs: status[p] (MPC_VX_*), n_vert[p], n_ray[p]; vertices [sum n_vert][n_t] polytope by polytope, each polytope's in
 * lexicographic order; incidence [sum n_vert][4] 64-bit masks over the polytope's rows; rays [sum n_ray][n_t] (unit 2-norm,
 * lexicographic order).  MPC_VX_UNBOUNDED polytopes return their vertices and rays; NOT_POINTED (rank E < n_t), EMPTY (no interior:
 * empty or lower dimensional) and OVERFLOW return none.  Two runs give the same bits.
 * Limits (MPC_ERR_INVALID with a message, before any launch): 1 <= n_t <= 16, <= 256 rows per polytope, finite rows, tol >= 0,
 * 18 <= slab <= max_slab <= 2^24, a budget that holds one polytope's first slab. */
#define MPC_VX_OK 0
#define MPC_VX_UNBOUNDED 1
#define MPC_VX_NOT_POINTED 2
#define MPC_VX_EMPTY 3
#define MPC_VX_OVERFLOW 4
typedef struct mpc_vertex_stats {
    int64_t generators;   /* generators made (initial ones included), over all passes */
    int64_t max_list;     /* the longest intermediate generator list */
    int64_t merges;       /* vertices merged into a neighbour within tol */
    int64_t repeats;      /* polytopes repeated with a larger slab */
    int64_t overflow;     /* polytopes left MPC_VX_OVERFLOW */
    int64_t launches;     /* launches of k_region_vertices */
    int64_t slab;         /* generators per list of the last pass */
    float ms;             /* device milliseconds of k_region_vertices */
} mpc_vertex_stats;
int mpc_region_vertices(int32_t device, int32_t n_t, int64_t n_poly, const int64_t *row_off, const double *ef_rows, double tol, int64_t slab,
                        int64_t max_slab, int64_t budget, int64_t *v_cap, int64_t *r_cap, int32_t *status, int64_t *n_vert, int64_t *n_ray,
                        double *vertices, uint64_t *incidence, double *rays, mpc_vertex_stats *stats);

/* ---- volumes and centroids of a batch of polytopes (geometry.polytope_volumes, Solution.volumes) ------------------------ */
/* mpc_region_volumes: the volume and the centroid of every polytope {theta : E theta <= f} from what mpc_region_vertices returned for the
 * same rows: vert_off[n_poly + 1] (the running sums of n_vert), vertices, incidence and vx_status.  The boundary triangulation of Cohen &
 * Hickey on the face lattice the incidence masks give (volume.hpp): the vertices are taken in the order they arrive, the apex of a
 * face is its lowest vertex, and every simplex adds |det| / n_t! and that times the mean of its points.  One wavefront per (polytope,
 * row); the sums of the waves are added in row order by a second kernel, so two runs give the same bits.
 *   ef_rows        [rows][n_t + 1]: only its row counts and its finiteness are used
 *   tol            the tolerance the incidence was computed with; checked, not applied again
 *   max_simplices  the most simplices one polytope may take (>= 1); a polytope over it ends MPC_VOL_TOO_LARGE, as does one of more than
 *                  16,384 vertices (the stack of a wave lives in LDS)
 *   budget         device bytes of the row-to-vertex bitsets in flight (<= 0: 4 GiB); polytopes run in chunks that fit
 * Outputs per polytope: status (MPC_VOL_*), volume, centroid [n_t], n_simplices (0 unless MPC_VOL_OK).
 *   vx_status EMPTY -> EMPTY, 0, NaN;  UNBOUNDED / NOT_POINTED -> the same status, +inf, NaN;  OVERFLOW -> OVERFLOW, NaN, NaN;
 *   MPC_VOL_TOO_LARGE and MPC_VOL_INCONSISTENT (a face without a facet, an edge without two ends: the incidence masks were blurred by
 *   a vertex merge) -> NaN, NaN, never a partial sum.
 * Limits (MPC_ERR_INVALID with a message, before any launch): 1 <= n_t <= 16, <= 256 rows per polytope, finite rows and vertices,
 * tol >= 0, max_simplices >= 1, a budget that holds one polytope. */
#define MPC_VOL_OK 0
#define MPC_VOL_UNBOUNDED 1
#define MPC_VOL_NOT_POINTED 2
#define MPC_VOL_EMPTY 3
#define MPC_VOL_OVERFLOW 4
#define MPC_VOL_TOO_LARGE 5
#define MPC_VOL_INCONSISTENT 6
typedef struct mpc_volume_stats {
    int64_t simplices;          /* simplices of all MPC_VOL_OK polytopes */
    int64_t max_simplices;      /* the most of one polytope */
    int64_t launches;           /* kernel launches */
    int64_t status_counts[7];   /* polytopes per MPC_VOL_* */
    float ms;                   /* device milliseconds of the three kernels */
} mpc_volume_stats;
int mpc_region_volumes(int32_t device, int32_t n_t, int64_t n_poly, const int64_t *row_off, const double *ef_rows, const int64_t *vert_off,
                       const double *vertices, const uint64_t *incidence, const int32_t *vx_status, double tol, int64_t max_simplices,
                       int64_t budget, double *volume, double *centroid, int64_t *n_simplices, int32_t *status, mpc_volume_stats *stats);

/* ---- second moments of a batch of polytopes (geometry.polytope_moments, Solution.moments) ------------------------------ */
/* mpc_region_moments: mpc_region_volumes with one more output, second_moment [n_poly][n_t][n_t], the integral of theta theta^T over every
 * polytope (symmetric, both triangles written).  The same walk with one more sum per wave (volume.hpp, M2 = true): every simplex adds
 * |det| / (n_t! (n_t + 1)(n_t + 2)) (sum_i v_i v_i^T + s s^T), s the sum of its vertices.  No floating-point atomics; volume, centroid,
 * n_simplices and status are bit for bit those of mpc_region_volumes for the same arguments.
 *   second_moment by status: MPC_VOL_OK -> the integral;  EMPTY -> zeros;  every other status -> NaN, never a partial sum.
 *   budget         also counts the second-moment slots, n_t (n_t + 1) / 2 doubles per row
 * The limits, the statuses and the statistics are those of mpc_region_volumes. */
int mpc_region_moments(int32_t device, int32_t n_t, int64_t n_poly, const int64_t *row_off, const double *ef_rows, const int64_t *vert_off,
                       const double *vertices, const uint64_t *incidence, const int32_t *vx_status, double tol, int64_t max_simplices,
                       int64_t budget, double *volume, double *centroid, int64_t *n_simplices, int32_t *status, double *second_moment,
                       mpc_volume_stats *stats);

/* ---- merging regions with equal laws into convex unions (Solution.merge_regions) --------------------------------- */
/* Regions are polytopes {theta : n.theta <= o} of unit rows: ef_rows [rows][n_t + 1] = [o | n] (|n| = 1 within 1e-6, finite), CSR over
 * regions by row_off[n_regions + 1] (row_off[0] = 0).  Limits (MPC_ERR_INVALID with a message, before any launch): 1 <= n_t <= 16,
 * 1..256 rows per region.
 *
 * mpc_merge_regions: a feasible point xs [n_regions][n_t] and the bounding box box [n_regions][2][n_t] (lower, upper; -inf / +inf
 *   where unbounded) of every region, one wavefront each (k_merge_regions); status[j] = 1 for an empty region (its box is +inf / -inf).
 *   stats (may be NULL): [0] LPs, [1] pivots, [2] LP runs stopped at the pivot cap.  ms (may be NULL): device milliseconds.
 * mpc_merge_pairs: the convexity test of P u Q for every pair (P, Q) = (pair_a[k], pair_b[k]) (k_merge_pairs), from the xs and box of
 *   mpc_merge_regions.  Row r of P is valid for Q iff max over Q of (n_r.theta - o_r) <= tol max(1, |o_r|) (bit r of
 *   env_a[k][0 .. MPC_MERGE_WORDS)), and the same for Q's rows over P (env_b).  verdict[k] = 1 iff every LP
 *   max t s.t. theta in the valid rows widened by tol max(1, |o|), n_i.theta - o_i >= t, n_j.theta - o_j >= t over the non-valid rows
 *   i of P and j of Q has t* <= tol (the union is then the valid rows); t_max[k]: the largest t reached (-inf: no such LP).  An
 *   unbounded or capped LP counts as "not valid" / "not convex".  Deterministic: atomics only in the counters.
 *   stats (may be NULL): [0] pairs, [1] pairs whose valid rows needed no LP, [2] rows tested, [3] rows decided without an LP, [4] LPs,
 *   [5] pivots, [6] capped runs. */
#define MPC_MERGE_WORDS 4
#define MPC_MERGE_MAX_ROWS 256
int mpc_merge_regions(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, double *xs, double *box,
                      int32_t *status, int64_t *stats, float *ms);
int mpc_merge_pairs(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *xs,
                    const double *box, int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, double tol, uint64_t *env_a,
                    uint64_t *env_b, int32_t *verdict, double *t_max, int64_t *stats, float *ms);

/* ---- overlap removal by lowest objective (Solution.remove_overlaps) ------------------------------------------------- */
/* Regions and pieces are polytopes of unit rows [o | n] in CSR form, as for the merge calls above.  Both calls are stateless; an error
 * text is read with mpc_last_error(NULL).  Limits (MPC_ERR_INVALID with a message, before any launch): 1 <= n_t <= 16, 1..256 rows per
 * region and per piece, finite rows with unit normals, indices in range, finite xs / start, tol finite and >= 0.
 *
 * mpc_overlap_pairs: for every pair (i, j) = (pair_a[k], pair_b[k]) over the rows of R_i and R_j together (k_overlap_pairs)
 *   radius[k]  the largest t with n.theta + t <= o for every row: the Chebyshev radius of R_i n R_j (negative: empty); the run starts
 *              at xs[i] (any finite point; a point of R_i saves pivots)
 *   d_min[k], d_max[k]  where radius[k] > tol and has_cut[k]: the range over R_i n R_j of d(theta) = o - n.theta for the cut row
 *              [o | n] = cut_rows[k] (the unit row of {J_j <= J_i}: d = (J_i - J_j) / |g|).  NaN where not computed.
 *   flag[k]    1: a run was unbounded or stopped at the pivot cap (radius, d_min, d_max are then bounds, not values)
 *   cut_rows may be NULL when no has_cut[k] is set.  stats (may be NULL): [0] pairs, [1] LPs, [2] pivots, [3] capped runs.
 * mpc_overlap_split: one step of the region difference for every item k = (piece item_piece[k], cutter region item_cutter[k], and the
 *   cut row cut_rows[k] where has_cut[k]); the cutter C is the region's rows followed by the cut row (k_overlap_split)
 *   flag[k]    bit 0 (MPC_OVERLAP_MEETS): radius(P n C) > tol.  Clear: the piece stays whole and nothing else is set.
 *              bit 1 (MPC_OVERLAP_CUT_ROW): the cut row cuts.  bit 2 (MPC_OVERLAP_WIDE): some run was unbounded or capped.
 *   mask[k][MPC_MERGE_WORDS]  bit r: row r of the cutter's region cuts, i.e. P n {earlier cutting rows} n {n_r.theta >= o_r} has a radius
 *              above tol, taken in row order; every such set is a child piece (rows: P's, the earlier cutting rows, the reversed row)
 *              and P n C is dropped.  An unbounded or capped run counts as "cuts".
 *   start      [n_items][n_t] where the first run of an item starts, or NULL: the origin.
 *   stats (may be NULL): [0] items, [1] items whose piece meets the cutter, [2] LPs, [3] pivots, [4] unbounded or capped runs.
 * Deterministic: atomics only in the counters. */
#define MPC_OVERLAP_MEETS 1
#define MPC_OVERLAP_CUT_ROW 2
#define MPC_OVERLAP_WIDE 4
int mpc_overlap_pairs(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *xs,
                      int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, const int32_t *has_cut, const double *cut_rows,
                      double tol, double *radius, double *d_min, double *d_max, int32_t *flag, int64_t *stats, float *ms);
int mpc_overlap_split(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, int64_t n_pieces,
                      const int64_t *piece_off, const double *piece_rows, int64_t n_items, const int32_t *item_piece,
                      const int32_t *item_cutter, const int32_t *has_cut, const double *cut_rows, const double *start, double tol,
                      int32_t *flag, uint64_t *mask, int64_t *stats, float *ms);

/* ---- the largest gap between two affine laws over region pairs (Solution.compare) --------------------------------- */
/* Regions are polytopes of unit rows [o | n] in CSR form, as for the merge and overlap calls above: ONE table, in which the caller
 * concatenates the regions of both solutions.  laws is n_regions x n_out x (n_t + 1) row-major, row k of region i = [b_i[k] | A_i[k]]:
 * the law x_k = A_i[k].theta + b_i[k] on the n_out output rows both sides are compared on.  xs (n_regions x n_t) is a point of every
 * region, from mpc_merge_regions.  Stateless; an error text is read with mpc_last_error(NULL).
 *
 * mpc_law_gap_pairs: for every pair (i, j) = (pair_a[k], pair_b[k]) (k_law_gap, one wavefront per pair):
 *   radius[k]  the Chebyshev radius of X = R_i n R_j, the run started at xs[i] and taken to its optimum.  radius <= tol: the pair does not
 *              meet (facet neighbours and disjoint regions): gap[k] NaN, gap_row[k] -1, witness and range NaN, flag 0, no law LP.
 *   otherwise, with delta_r(theta) = (A_i[r] - A_j[r]).theta + (b_i[r] - b_j[r]) for output row r, lo_r = min and hi_r = max of delta_r
 *   over X: 2 LPs per row in the fixed order row 0 min, row 0 max, row 1 min, ..., each warm-started where the previous one ended, the
 *   first from the Chebyshev centre.  A row with A_i[r] == A_j[r] in every entry (compared as doubles, no threshold) is constant:
 *   lo_r = hi_r = b_i[r] - b_j[r] and no LP runs.
 *   gap[k]     max_r max(-lo_r, hi_r) >= 0.   gap_row[k]: the lowest r that attains it.   witness[k][n_t]: the theta where that run ended
 *              (the Chebyshev centre when a constant row gives the gap).   range (may be NULL) [k][n_out][2] = lo_r, hi_r.
 *   flag[k]    1: a bound, not a value.  A radius run that is unbounded (radius +inf) or stopped at the pivot cap (radius: the value
 *              reached) gives gap +inf, gap_row -1, range NaN, witness the point reached, and no law LP.  A law LP that is unbounded or
 *              capped gives lo_r = -inf or hi_r = +inf, hence gap +inf.
 *   pair_a[k] == pair_b[k] is legal (gap 0).  n_pairs == 0: MPC_OK without a launch.
 *   stats (may be NULL): [0] pairs, [1] pairs that meet, [2] constant rows (no LP), [3] LPs, [4] pivots, [5] unbounded or capped runs.
 * MPC_ERR_INVALID with a message, before a device is selected: a missing array, 1 <= n_t <= 16, 1 <= n_out <= 256, 1..256 rows per region,
 * finite rows with unit normals, finite laws and xs, tol finite and >= 0, n_pairs in 0..2^31 - 1, pair indices in range.
 * Deterministic: atomics only in the counters, no floating-point atomics. */
int mpc_law_gap_pairs(int32_t device, int32_t n_t, int32_t n_out, int64_t n_regions, const int64_t *row_off, const double *ef_rows,
                      const double *laws, const double *xs, int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, double tol,
                      double *radius, double *gap, int32_t *gap_row, double *witness, double *range, int32_t *flag, int64_t *stats,
                      float *ms);

/* ---- the candidate sweep over bounding boxes and the row screen behind it (geometry.box_pairs) ---------------------- */
/* Boxes are n x 2 x n_t row-major (lower bounds, then upper bounds) with one usable byte per box.  A NaN lower bound reads as -inf, a NaN
 * upper bound as +inf.  Stateless; an error text is read with mpc_last_error(NULL).
 *
 * mpc_box_pairs: the pairs (i, j), i a box of family a in the row range [i0, i1), j a box of family b, both usable, with
 *     min(hi_a[i][k], hi_b[j][k]) - max(lo_a[i][k], lo_b[j][k]) > margin      for every coordinate k,
 *   evaluated in fp64 exactly as written (one subtraction, a strict compare; infinities are ordinary values, an inf - inf that gives
 *   NaN fails).  mode MPC_BOX_CROSS: every (i, j), i == j included.  MPC_BOX_UPPER: family a against itself, i < j only; family b is left
 *   out (n_b = 0, NULL) or names family a again.
 *   total      the number of pairs of the range; always written.
 *   pair_a, pair_b [cap]  the pairs, ascending by (i, j), written iff 0 < total <= cap: a list that does not fit is not written at all
 *              and the caller repeats the call with cap >= total.  cap == 0 with NULL pointers is the count-only call.
 *   row_count  (may be NULL) [i1 - i0] the pairs of every row of the range.
 *   The order comes from the construction (k_box_pairs counts per (row, segment of family b), an exclusive scan gives every cell its
 *   offset, a second pass writes in place): no sort, no atomic, two calls give the same bytes.
 *   stats (may be NULL): [0] box tests (usable a in the range x usable b; UPPER: the usable j > i behind every usable i of the range),
 *   [1] pairs, [2] segments of family b.  A family (or range) without a usable box: total 0 without a launch.
 * MPC_ERR_INVALID with a message, before a device is selected: a missing array, 1 <= n_t <= 16, an unknown mode, a family with no box,
 * UPPER with two different families, a row range outside 0 <= i0 <= i1 <= n_a, cap < 0, a margin that is not finite.
 *
 * mpc_pair_screen: regions are polytopes of unit rows [o | n] in CSR form, as for the merge and overlap calls above.  For every candidate
 *   (i, j) = (pair_a[k], pair_b[k]) and every screened side (sides: MPC_SCREEN_ROWS_A, MPC_SCREEN_ROWS_B or both): side A tests the rows of
 *   region i against box_for_a_rows[j], side B the rows of region j against box_for_b_rows[i]; both tables are n_regions x 2 x n_t, and
 *   the one of a side that is not screened may be NULL.  With s = sum over ascending k of n_k (lo[k] if n_k > 0 else hi[k]), terms with
 *   n_k == 0 skipped, the least value of n.theta on the box, a row separates when s - o > 1e-12 (1 + |o|); keep[k] = 0 iff some row
 *   separates (k_pair_screen, one lane per candidate).  A separated pair has an empty intersection whenever the box contains the set
 *   it stands for.  stats (may be NULL): [0] pairs, [1] dropped, [2] rows read.
 * MPC_ERR_INVALID as for mpc_merge_pairs, plus sides outside 1..3 and candidate indices out of range.  n_pairs == 0: MPC_OK without a
 * launch.  Deterministic: atomics only in the counters. */
#define MPC_BOX_CROSS 0
#define MPC_BOX_UPPER 1
#define MPC_SCREEN_ROWS_A 1
#define MPC_SCREEN_ROWS_B 2
int mpc_box_pairs(int32_t device, int32_t n_t, int32_t mode, int64_t n_a, const double *box_a, const uint8_t *usable_a, int64_t n_b,
                  const double *box_b, const uint8_t *usable_b, double margin, int64_t i0, int64_t i1, int64_t cap, int64_t *pair_a,
                  int64_t *pair_b, int64_t *row_count, int64_t *total, int64_t *stats, float *ms);
int mpc_pair_screen(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, int64_t n_pairs,
                    const int64_t *pair_a, const int64_t *pair_b, const double *box_for_a_rows, const double *box_for_b_rows, int32_t sides,
                    uint8_t *keep, int64_t *stats, float *ms);

/* ---- transition graph of a closed loop between regions (Solution.transition_graph) --------------------------------- */
/* Regions are polytopes of unit rows [o | n] in CSR form, as for the merge and overlap calls above; region i has the closed-loop map
 * theta+ = Phi_i theta + phi_i (Phi n_regions x n_t x n_t row-major, phi n_regions x n_t).  xs (n_regions x n_t) is a point of every
 * region, from mpc_merge_regions.  Both calls are stateless; an error text is read with mpc_last_error(NULL).  MPC_ERR_INVALID with a
 * message, before a device is selected: a missing array, 1 <= n_t <= 16, 1..256 rows per region, finite rows with unit normals, finite
 * Phi, phi, xs, tol finite and >= 0, n_pairs in 0..2^31 - 1, pair indices in range (pair_a[k] == pair_b[k] is legal: a self loop).
 *
 * mpc_transition_boxes: image_box n_regions x 2 x n_t (lower, upper), the exact bounding box of Phi_i R_i + phi_i (k_transition_boxes);
 *   -inf / +inf where the image is unbounded or the run stopped at the pivot cap; flag[i] = 1: some run of region i was capped.
 *   stats (may be NULL): [0] LPs, [1] pivots, [2] capped runs.
 * mpc_transition_pairs: for every pair (i, j) = (pair_a[k], pair_b[k]) the Chebyshev radius of T_ij = {theta in R_i : Phi_i theta + phi_i
 *   in R_j}, over the rows of R_i and the rows of R_j pulled back through the map of i and scaled to unit normals (k_transition_pairs).
 *   A pulled-back row whose normal is no longer than 1e-12 max(1, max |Phi_i|) is constant: it empties T_ij when its right-hand side is
 *   below -tol (radius -inf, no LP) and is dropped otherwise.
 *   full_radius != 0: the run goes to the optimum; 0: it stops once the radius exceeds tol (radius[k] is then a lower bound above tol).
 *   status[k]  MPC_TRANSITION_NO_EDGE (radius <= tol), _EDGE, _UNBOUNDED (an edge, radius +inf), _UNDECIDED (the run stopped at the pivot
 *              cap; kept as an edge by the host).  witness[k][n_t]: the theta where the run ended.
 *   n_pairs == 0: MPC_OK without a launch.  stats (may be NULL): [0] pairs, [1] LPs, [2] pivots, [3] capped runs.
 * Deterministic: atomics only in the counters. */
#define MPC_TRANSITION_NO_EDGE 0
#define MPC_TRANSITION_EDGE 1
#define MPC_TRANSITION_UNBOUNDED 2
#define MPC_TRANSITION_UNDECIDED 3
int mpc_transition_boxes(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *Phi,
                         const double *phi, const double *xs, double *image_box, int32_t *flag, int64_t *stats, float *ms);
int mpc_transition_pairs(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *Phi,
                         const double *phi, const double *xs, int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b,
                         int32_t full_radius, double tol, double *radius, int32_t *status, double *witness, int64_t *stats, float *ms);

/* ---- exit sets of a closed loop (Solution.exit_sets) ---------------------------------------------------------------- */
/* Regions, maps and pieces as for the overlap and transition calls above.  Stateless; an error text is read with mpc_last_error(NULL).
 * MPC_ERR_INVALID with a message, before a device is selected: a missing array, 1 <= n_t <= 16, 1..256 rows per region and per piece,
 * finite rows with unit normals, finite Phi, phi, start, tol finite and >= 0, n_items in 0..2^31 - 1, indices in range.
 *
 * mpc_exit_split: one step of the region difference for every item k = (piece item_piece[k], source region i = item_source[k], target
 *   region j = item_target[k]).  The cutter is C_ij = {theta : Phi_i theta + phi_i in R_j}: the rows of R_j pulled back through the map
 *   of i exactly as mpc_transition_pairs forms them (a constant row with right-hand side below -tol empties C_ij: the piece stays and no
 *   LP runs; any other constant row is dropped and never cuts) (k_exit_split).
 *   flag[k]    bit 0 (MPC_OVERLAP_MEETS): radius(P n C_ij) > tol.  Clear: the piece stays whole and the mask is empty.
 *              bit 2 (MPC_OVERLAP_WIDE): some run was unbounded or capped.  Bit 1 is never set.
 *   mask[k][MPC_MERGE_WORDS]  bit r: row r of region j, pulled back, cuts, i.e. P n {earlier cutting rows} n {the reversed row} has a
 *              radius above tol, taken in row order; every such set is a child piece (rows: P's, the earlier cutting pulled-back rows,
 *              the reversed one) and P n C_ij is dropped.  An unbounded or capped run counts as "cuts".
 *   start      [n_items][n_t] where the first run of an item starts, or NULL: the origin.
 *   n_items == 0: MPC_OK without a launch.
 *   stats (may be NULL): [0] items, [1] items whose piece meets the cutter, [2] LPs, [3] pivots, [4] unbounded or capped runs.
 * Deterministic: atomics only in the counters. */
int mpc_exit_split(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *Phi,
                   const double *phi, int64_t n_pieces, const int64_t *piece_off, const double *piece_rows, int64_t n_items,
                   const int32_t *item_piece, const int32_t *item_source, const int32_t *item_target, const double *start, double tol,
                   int32_t *flag, uint64_t *mask, int64_t *stats, float *ms);

/* ---- redundant rows of polytopes (geometry.reduce_rows_of) ----------------------------------------------------------- */
/* Polytopes as unit rows [o | n] in CSR form by row_off, as above, but up to MPC_REDUCE_MAX_ROWS rows each.  Stateless; an error text is
 * read with mpc_last_error(NULL).  MPC_ERR_INVALID with a message, before a device is selected: a missing array, 1 <= n_t <= 16, 1..512
 * rows per polytope, finite rows with unit normals, finite start, tol finite and >= 0, n_poly in 0..2^31 - 1, row_off non-decreasing from 0.
 *
 * mpc_reduce_rows: the sequential rule for every polytope P (k_reduce_rows).  radius(P) <= tol: P is thin, status MPC_REDUCE_THIN, every
 *   mask bit set, no row tested.  Otherwise for k = 0 .. m - 1 in order: row k is redundant iff the rows still live (the kept rows before k
 *   and all rows after k) together with the reversed row {n_k.theta >= o_k} have a Chebyshev radius <= tol; a redundant row is removed at
 *   once.  A run that is unbounded or stopped at the pivot cap counts as "kept".
 *   status[q]  MPC_REDUCE_OK or MPC_REDUCE_THIN.   wide[q]: the number of unbounded or capped runs of polytope q.
 *   kept[q][MPC_REDUCE_WORDS]  bit k: row k stays.
 *   start      [n_poly][n_t] where the first run of a polytope starts, or NULL: the origin.
 *   point      [n_poly][n_t] or NULL: where the first run ended (interior when it was neither thin nor wide), the start of every row run.
 *   n_poly == 0: MPC_OK without a launch.
 *   stats (may be NULL): [0] polytopes, [1] thin ones, [2] LPs, [3] pivots, [4] unbounded or capped runs.
 * Deterministic: atomics only in the counters. */
#define MPC_REDUCE_MAX_ROWS 512
#define MPC_REDUCE_WORDS 8
#define MPC_REDUCE_OK 0
#define MPC_REDUCE_THIN 1
int mpc_reduce_rows(int32_t device, int32_t n_t, int64_t n_poly, const int64_t *row_off, const double *ef_rows, const double *start, double tol,
                    int32_t *status, int32_t *wide, uint64_t *kept, double *point, int64_t *stats, float *ms);

/* ---- support functions of polytopes (geometry.support_of) ------------------------------------------------------------ */
/* Polytopes as unit rows [o | n] in CSR form by row_off, 1..MPC_SUPPORT_MAX_ROWS rows each, as for mpc_reduce_rows.  Directions in a second
 * CSR table: polytope q owns the rows dir_off[q] .. dir_off[q + 1] of dirs [n_dir][n_t]; a polytope without directions is legal.  Stateless;
 * an error text is read with mpc_last_error(NULL).
 *
 * mpc_support_rows: h_P(d) = max {d.x : x in P} for every polytope P and each of its directions d (k_support_rows; one wavefront per block
 *   of 64 consecutive directions of one polytope, the blocks listed by the call itself).
 *   Interior point: the radius run of mpc_reduce_rows from start, stopped once t > tol.  Optimal with t <= tol: P is thin, poly_status
 *   MPC_SUPPORT_THIN, and every direction of P gets value = arg = NaN and dir_status MPC_SUPPORT_THIN without an LP.  Otherwise the point p
 *   where the run ended.  An unbounded or capped radius run is not thin and sets wide[q] = 1: an unbounded run (it ends while t <= tol,
 *   where the point need not lie in P) moves p along the ray it found to t = tol + 1, a point of P of that radius; a capped run with
 *   t >= 0 goes on from the point reached; a capped run with t < 0 knows no point of P, and every direction of P gets value +inf, arg NaN
 *   and MPC_SUPPORT_CAPPED without an LP.
 *   One direction: d == 0 in every entry: value 0, arg p, MPC_SUPPORT_OK, no LP.  Otherwise max c.x, c = d / |d| (d scaled by a power of
 *   two first, so that no finite direction overflows or underflows), by the vertex simplex
 *   from p with a fresh basis.  Optimal: arg is the point reached and value = d.arg (fma over ascending t), MPC_SUPPORT_OK.  Unbounded:
 *   value +inf, arg the last point reached, MPC_SUPPORT_UNBOUNDED.  Pivot cap: value +inf, a bound and not a value, MPC_SUPPORT_CAPPED.
 *   Every run starts from p alone, so the result of a direction depends on (rows, start, tol, d) only: permuting a polytope's directions
 *   or repeating one changes no bit of any result.
 *   value [n_dir], dir_status [n_dir], arg [n_dir][n_t] or NULL.
 *   poly_status[q]  MPC_SUPPORT_OK or MPC_SUPPORT_THIN.   wide[q]: 1 when the radius run of q was unbounded or capped.
 *   start      [n_poly][n_t] where the radius run of a polytope starts, or NULL: the origin.
 *   point      [n_poly][n_t] or NULL: where the radius run ended, the p above.
 *   n_poly == 0: MPC_OK without a launch.  No direction at all: one launch for poly_status, wide and point.
 *   stats (may be NULL): [0] polytopes, [1] thin ones, [2] directions, [3] zero directions, [4] LPs (one radius run per polytope and one
 *   run per direction that is not zero), [5] pivots, [6] unbounded or capped runs.
 * MPC_ERR_INVALID with a message, before a device is selected: a missing array, 1 <= n_t <= 16, 1..512 rows per polytope, finite rows with
 * unit normals, dir_off non-decreasing from 0, at most 2^31 - 1 polytopes, directions and blocks, finite directions, finite start, tol
 * finite and >= 0.  Deterministic: atomics only in the counters. */
#define MPC_SUPPORT_MAX_ROWS 512
#define MPC_SUPPORT_OK 0
#define MPC_SUPPORT_UNBOUNDED 1
#define MPC_SUPPORT_CAPPED 2
#define MPC_SUPPORT_THIN 3
int mpc_support_rows(int32_t device, int32_t n_t, int64_t n_poly, const int64_t *row_off, const double *ef_rows, const int64_t *dir_off,
                     const double *dirs, const double *start, double tol, double *value, double *arg, int32_t *dir_status,
                     int32_t *poly_status, int32_t *wide, double *point, int64_t *stats, float *ms);

/* ---- projections of polytopes (geometry.project_rows_of) -------------------------------------------------------------- */
/* Polytopes of R^n as unit rows [o | n] in CSR form by row_off, up to MPC_PROJECT_MAX_ROWS rows each.  Stateless; an error text is read
 * with mpc_last_error(NULL).
 *
 * mpc_project_rows: the projection of every polytope onto its first n - n_elim coordinates (k_project_rows), by Fourier-Motzkin
 *   elimination of the trailing n_elim coordinates, the last one first, every step followed by the sequential rule of mpc_reduce_rows.
 *   First the radius run of mpc_reduce_rows from start: radius <= tol, MPC_PROJECT_THIN.  A step eliminates coordinate j, the last one
 *   left, over the live rows in order; c is a row's coefficient of j, Z: |c| <= 1e-12, P: c > 1e-12, N: c < -1e-12.  The new rows: the
 *   rows of Z in order without column j (scaled to a unit normal again unless c == 0), then for p over P in order and q over N in order
 *   inside it (-c_q) row_p + c_p row_q without column j, scaled to a unit normal.  A combination whose normal has a norm <= 1e-9 before
 *   scaling says 0 <= rhs: it is dropped, or with rhs < -tol the polytope is empty, MPC_PROJECT_THIN.  With P or N empty the rows of Z
 *   alone are kept; no row left: MPC_PROJECT_WHOLE (the whole space).  |Z| + |P||N| > 512: MPC_PROJECT_TOO_LARGE.  Then the interior
 *   point loses coordinate j, the radius run from it (radius <= tol: MPC_PROJECT_THIN), and the sequential rule over the new rows, every
 *   run started where that run ended; the kept rows, in order, are the live rows of the next step.  A run that is unbounded or stopped at
 *   the pivot cap counts as "kept".  n_elim == 0: one pass of mpc_reduce_rows, the kept rows returned.
 *   status[q]  MPC_PROJECT_OK, _THIN, _WHOLE or _TOO_LARGE (a step above 512 rows, or more than out_cap rows at the end); only
 *              MPC_PROJECT_OK returns rows: n_out[q] of them in out_rows[q][out_cap][n - n_elim + 1], unit rows [o | n], zeros behind them; the
 *              others have n_out[q] = 0.
 *   wide[q]    the number of unbounded or capped runs of polytope q.   peak[q] (may be NULL): the largest |Z| + |P||N| of its steps.
 *   start      [n_poly][n] where the first run of a polytope starts, or NULL: the origin.
 *   point      [n_poly][n - n_elim] or NULL: the interior point of the result (MPC_PROJECT_OK; zeros otherwise).
 *   n_poly == 0: MPC_OK without a launch.
 *   stats (may be NULL): [0] polytopes, [1] thin, [2] whole, [3] too large, [4] steps, [5] rows made, [6] LPs, [7] pivots, [8] unbounded
 *   or capped runs.
 * MPC_ERR_INVALID with a message, before a device is selected: a missing array, 1 <= n <= 16, 0 <= n_elim <= n - 1, 1..512 rows per
 * polytope, finite rows with unit normals, finite start, tol finite and >= 0, 1 <= out_cap <= 512, n_poly in 0..2^31 - 1, row_off
 * non-decreasing from 0.  Deterministic: atomics only in the counters. */
#define MPC_PROJECT_MAX_ROWS 512
#define MPC_PROJECT_OK 0
#define MPC_PROJECT_THIN 1
#define MPC_PROJECT_WHOLE 2
#define MPC_PROJECT_TOO_LARGE 3
int mpc_project_rows(int32_t device, int32_t n, int32_t n_elim, int64_t n_poly, const int64_t *row_off, const double *ef_rows,
                     const double *start, double tol, int32_t out_cap, double *out_rows, int32_t *n_out, int32_t *status, int32_t *wide,
                     int32_t *peak, double *point, int64_t *stats, float *ms);

/* ---- backward exit cells of a closed loop (Solution.invariant_set) --------------------------------------------------- */
/* Regions and maps as for the transition and exit calls above; xs [n_regions][n_t] is a feasible point of every region (mpc_merge_regions).
 * A CELL is a polytope of 1..256 unit rows that lies in region source[c].  The cells of step 0 are given (the exit pieces of
 * Solution.exit_sets); a cell of step k + 1 is R_i n f_i^-1(Q) for a cell Q of step k and a region i of pred_idx[pred_off[j] ..
 * pred_off[j + 1]), j = source(Q): the states of R_i whose next state lies in Q.  Stateless; an error text is read with mpc_last_error(NULL).
 *
 * mpc_backward_exits runs every step itself.  The items of a step are ordered by parent cell, then as the predecessor list is; per item
 *   (k_pre_cells, one wavefront): the rows of Q pulled back through the map of i exactly as mpc_transition_pairs forms them (a constant row
 *   with right-hand side below -tol: no cell and no LP; any other constant row is dropped); the radius of R_i's rows and the pulled-back
 *   ones from xs[i], stopped once it exceeds tol (optimal and not above tol: no cell; unbounded or capped: a cell, flagged wide: it may hold states that stay); for a cell
 *   the sequential rule of mpc_reduce_rows over R_i's rows, then the pulled-back ones, every run started where the radius run ended.  The
 *   kept rows become the cell (k_pre_emit), appended to the cell table ON THE DEVICE: between steps only per-item status words and counts
 *   come to the host, which scans the offsets and lists the next items.  The iteration ends when a step yields no cell.
 *   max_steps        at most so many steps are run (>= 0).  max_cells, max_rows_total: the capacity of the output arrays, step 0 included.
 *   n_cells, cell_off [n_cells + 1], cell_rows [cell_off[n_cells]][n_t + 1], cell_source, cell_step, cell_parent (-1 at step 0, else the
 *   index of Q), cell_wide (its own radius run or an ancestor's was unbounded or capped): all cells, step by step, a step in item order.
 *   cell_point       [max_cells][n_t] or NULL: for the cells of the steps >= 1, where the radius run ended (rows of step 0 are not written).
 *   status           MPC_BACKWARD_CONVERGED; MPC_BACKWARD_MAX_STEPS: max_steps steps were run and the last one had cells with
 *                    predecessors; MPC_BACKWARD_ROWS: a reduced cell keeps more than 256 rows; MPC_BACKWARD_MAX_CELLS,
 *                    MPC_BACKWARD_MAX_ROWS_TOTAL: a step did not fit.  After the last three the cells of the completed steps are returned.
 *   steps            the completed steps that yielded cells; converged: status == MPC_BACKWARD_CONVERGED.
 *   cells_per_step   [max_steps + 1]; step_ms [max_steps] (either may be NULL): device ms of step k + 1, the one that found nothing included.
 *   stats (may be NULL): [0] items, [1] cells found, [2] items emptied by a constant row, [3] LPs, [4] pivots, [5] unbounded or capped runs.
 *   n_cells0 == 0 or max_steps == 0: MPC_OK without a launch (step 0 is returned).
 * MPC_ERR_INVALID with a message, before a device is selected: everything mpc_exit_split refuses (cells for pieces), xs not finite, an index
 * out of range in pred_idx or cell_source0, pred_off not non-decreasing from 0, max_steps < 0, step 0 larger than max_cells or
 * max_rows_total, a missing array.  Deterministic: atomics only in the counters. */
#define MPC_BACKWARD_CONVERGED 0
#define MPC_BACKWARD_MAX_STEPS 1
#define MPC_BACKWARD_ROWS 2
#define MPC_BACKWARD_MAX_CELLS 3
#define MPC_BACKWARD_MAX_ROWS_TOTAL 4
int mpc_backward_exits(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *Phi,
                       const double *phi, const double *xs, const int64_t *pred_off, const int32_t *pred_idx, int64_t n_cells0,
                       const int64_t *cell_off0, const double *cell_rows0, const int32_t *cell_source0, double tol, int32_t max_steps,
                       int64_t max_cells, int64_t max_rows_total, int64_t *n_cells, int64_t *cell_off, double *cell_rows, int32_t *cell_source,
                       int32_t *cell_step, int32_t *cell_parent, int32_t *cell_wide, double *cell_point, int32_t *status, int32_t *steps,
                       int32_t *converged, int64_t *cells_per_step, float *step_ms, int64_t *stats, float *ms);

/* ---- forward cells of a closed loop (Solution.reach_cells) ------------------------------------------------------------ */
/* Regions and maps as above.  A CELL of step k is a polytope Q of 1..256 unit rows over the INITIAL state theta_0: the initial states whose
 * state at step k lies in region cell_region[c], where theta_k = G theta_0 + g with [G | g] = cell_map[c] ([n_t][n_t + 1]).  The cells of
 * step 0 are given, each inside its region, with an interior point each and the map [I | 0].  A cell of step k + 1 is
 * Q n {theta_0 : P theta_0 + s in R_j} for a cell Q of step k and a region j of succ_idx[succ_off[i] .. succ_off[i + 1]), i = region(Q),
 * under the NEXT MAP of Q, P = Phi_i G, s = Phi_i g + phi_i: every entry one sum over t ascending from 0.0 of plain IEEE products, so
 * the maps are the same bits wherever they are computed.  No map is inverted.  Stateless; an error text is read with mpc_last_error(NULL).
 *
 * mpc_forward_cells runs every step itself.  The items of a step are ordered by parent cell, then as the successor list is; per item
 *   (k_fwd_cells, one wavefront): the rows of R_j pulled back through the next map exactly as mpc_transition_pairs forms them (a constant
 *   row with right-hand side below -tol: no cell and no LP; any other constant row is dropped); the radius of Q's rows and the pulled-back
 *   ones from Q's point, stopped once it exceeds tol (optimal and not above tol: no cell; unbounded or capped: a cell, flagged wide, as is
 *   every descendant); for a cell the sequential rule of mpc_reduce_rows over Q's rows, then the pulled-back ones, every run started where
 *   the radius run ended.  The kept rows become the cell (k_fwd_emit), appended with point and map to the cell table ON THE DEVICE: between
 *   steps only per-item status words and counts come to the host, which scans the offsets and lists the next items.
 *   max_steps        so many steps are run (>= 0).  max_cells, max_rows_total: the capacity of the output arrays, step 0 included.
 *   n_cells, cell_off [n_cells + 1], cell_rows [cell_off[n_cells]][n_t + 1], cell_region, cell_step, cell_parent (-1 at step 0, else the
 *   index of Q), cell_wide, cell_point [max_cells][n_t] (step 0: as given; later: where the radius run ended), cell_map
 *   [max_cells][n_t][n_t + 1]: all cells, step by step, a step in item order.
 *   status           MPC_FORWARD_DONE: max_steps steps were run; MPC_FORWARD_EMPTY: a step yielded no cell, every trajectory has left;
 *                    MPC_FORWARD_ROWS: a reduced cell keeps more than 256 rows (or an item more than 512); MPC_FORWARD_MAX_CELLS,
 *                    MPC_FORWARD_MAX_ROWS_TOTAL: a step did not fit.  After the last three the cells of the completed steps are returned.
 *   steps            the completed steps.  cells_per_step [max_steps + 1]; step_ms [max_steps] (either may be NULL): device ms of step
 *                    k + 1, a step that found nothing or was refused included.
 *   stats (may be NULL): [0] items, [1] cells found, [2] items emptied by a constant row, [3] LPs, [4] pivots, [5] unbounded or capped runs.
 *   n_cells0 == 0 (MPC_FORWARD_EMPTY) or max_steps == 0 (MPC_FORWARD_DONE): MPC_OK without a launch (step 0 is returned).
 * MPC_ERR_INVALID with a message, before a device is selected: everything mpc_backward_exits refuses, with successor lists for
 * predecessor lists and without xs; cell_point0 missing or not finite.  Deterministic: atomics only in the counters. */
#define MPC_FORWARD_DONE 0
#define MPC_FORWARD_EMPTY 1
#define MPC_FORWARD_ROWS 2
#define MPC_FORWARD_MAX_CELLS 3
#define MPC_FORWARD_MAX_ROWS_TOTAL 4
int mpc_forward_cells(int32_t device, int32_t n_t, int64_t n_regions, const int64_t *row_off, const double *ef_rows, const double *Phi,
                      const double *phi, const int64_t *succ_off, const int32_t *succ_idx, int64_t n_cells0, const int64_t *cell_off0,
                      const double *cell_rows0, const int32_t *cell_region0, const double *cell_point0, double tol, int32_t max_steps,
                      int64_t max_cells, int64_t max_rows_total, int64_t *n_cells, int64_t *cell_off, double *cell_rows, int32_t *cell_region,
                      int32_t *cell_step, int32_t *cell_parent, int32_t *cell_wide, double *cell_point, double *cell_map, int32_t *status,
                      int32_t *steps, int64_t *cells_per_step, float *step_ms, int64_t *stats, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* MPCOMBI_H */
