// knobs.hpp -- every environment variable the library reads: one struct of values, one table of rows, one parser.
//
// Host-only plain C++17 (no HIP header: a host compiler builds it alone, tests/test_knobs_cpu.py does).  `Knobs` holds what a handle
// takes from the environment at its creation (Knobs::from_env(), called once by mpc_create's fill); its initialisers are the effective
// defaults.  The process-wide rows of the same table have no member: knob_process() reads one of them by name, at the moment its caller
// chooses -- that moment is behaviour and is named in the row.  std::getenv appears in csrc/ in this file only.  Every switch is an
// A/B or test lever; none is needed in production (INTEGRATION.md section 5 lists them for users, the test compares that list with this table).
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace mpc {
namespace {   // (internal linkage in each of the two units that include it: the library exports the C ABI and nothing of this)

struct Knobs {
    int x1_defer = 1;           // 1: k_x1 on its own stream from the plan pass on; 0: in line
    int xq_skip_below = 100000;  // the last level's product-form quick test leaves a list shorter than this to k_x2 when a tableau row is one lane's (MPC_XQ_SKIP_BELOW; 0: never).  Measured: config 3 (62 k left over) 4.26 -> 4.18 ms, config 4 (2.7 k) unchanged -- its last level ends with the region kernel
    int x_second_max = 1024;     // k_x2: a level's budget of doubtful cached runs repeated from D0 in the kernel (MPC_X_SECOND_MAX; 0: all go to the LDS engine)
    double x_fresh_limit = 1e6;   // k_x2: growth up to which a run from D0 decides (DictCache::fresh_limit; MPC_X_FRESH_LIMIT=0: GROWTH_SAFE)
    int kkt_spread_threads = 1 << 19;   // classic path: the spread form while candidates x KKT_SPREAD stays below this (MPC_KKT_SPREAD_THREADS)
    int kkt_spread = 1;         // small levels: k_kkt_thread with KKT_SPREAD lanes per candidate (MPC_KKT_SPREAD=0: one lane)
    // Round 6: the pruned list bucketed by smallest non-equality member (kernels.hpp, k_children_count_b), rebuilt at the start of every level
    // whose children stage is large enough to pay for it (MPC_PRUNED_BUCKET_MIN: parents x pruned sets; 0 = never)
    double pruned_bucket_min = 2.0e7;
    long long pruned_bucket_np = 1024;   // MPC_PRUNED_BUCKET_NP: ... and at least this many pruned sets (tests: 1)
    bool no_roverlap = false;        // MPC_NO_ROVERLAP=1 / mpc_set_region_overlap(h, 0): region stage after the (x,theta) stage (no overlap).  Written after creation by mpc_set_region_overlap
                                     // (it also keeps the region stage of a small level in line instead of beside the next level: mpc_handle::RegionDefer)
    int test_spare = 0;              // MPC_TEST_SPARE=N (tests): N fewer spare region slots than the overlapped launch would reserve
    int rsplit_max = 4;              // MPC_RSPLIT_MAX: most wavefronts that share one optimal candidate in k_region2 (power of two, <= 16; measured:
                                     // 8 and 16 shorten no level of config 4 or 2 -- every wavefront repeats the row build and the Chebyshev LP, 40 % of
                                     // a region at 4 -- and move the facet list of one sliver region)
    int xqg_per_cu = 4;              // MPC_XQG_PER_CU: workgroups (of four wavefronts) per CU of the persistent k_xq_grouped launch (default: XQG_WAVES of kernels2.hpp, asserted by the engine unit)
    int x2_wpc = 12, x2_div = 16, xq_wpc = 20;    // MPC_X2_WPC (most) / MPC_X2_DIV (items per wavefront) / MPC_XQ_WPC: wavefronts per CU of the persistent
                                     // k_x2 / k_xq launches (round 3: 16 and 32 whatever the size of the level).  x2_wpc is written after the parse by creation's
                                     // register-path stage: clamped for the 32-column instantiations of k_x2
    int r2_cap_pct = 100;            // MPC_R2_CAP: share (per cent) of k_region2's wave slots an overlapped one-wave-per-candidate launch may take
    bool test_small_fallback = false; // MPC_TEST_SMALL_FALLBACK=1 (tests): every level run without host round trips reports "repeat on the classic path"
    bool no_smallpath = false;       // MPC_NO_SMALLPATH=1: levels of any size take the classic path with its host round trips (A/B)
    long long smallpath_max = 4096;  // MPC_SMALLPATH_MAX: largest level (candidates) that runs without host round trips (measured: config 4 is
                                     // fastest with 1,024-4,096 -- a level of 15,691 candidates prefers the classic path, which streams its records)
    long long x_first_min = 4096, x_first_max = 65536;   // MPC_X_FIRST_MIN / _MAX: levels (candidates) whose (x,theta) stage is queued before the read-back.  Measured, config 4: level 3
                                     // (9,880 candidates) 0.72 -> 0.67 ms; level 4 (181 k) 1.51 -> 1.58: there the stage fills the GPU before the region kernel's long wavefronts are placed
                                     // (region kernel 0.48 -> 0.60 ms, the stage itself 0.93 -> 1.03) -- large levels keep the region launch first
    bool no_kkt_lists = false;       // MPC_NO_KKT_LISTS=1: the work lists behind k_kkt_thread by compaction of the status array (round 4; A/B, tests)
    bool no_small_rx = false;        // MPC_NO_SMALL_RX=1: region kernel and (x,theta) kernel of a small level as two launches (A/B, tests)
    bool no_small_fuse = false;      // MPC_NO_SMALL_FUSE=1: the small path with its round-4 launches (doubtful candidates re-solved in place; A/B, tests)
    long long roverlap_min = 2048, roverlap_long = 50000;   // MPC_ROVERLAP_MIN / MPC_ROVERLAP_LONG (items of the (x,theta) stage)
    int test_late = 0;               // MPC_TEST_LATE=N (tests): the overlapped launch leaves N optimal candidates to the late path
    int debug_cycles = 0;     // MPC_DEBUG_CYCLES=1: per-level cycle breakdown on stderr
    int no_rbox = 0;          // MPC_NO_RBOX=1: no bounding-box screen of the region rows in k_region2 (A/B)
    int no_rsplit = 0;        // MPC_NO_RSPLIT=1: one wavefront per candidate in k_region2 whatever the load (A/B)
    int x1 = 2;               // MPC_X1=0: every dictionary of a storing level by the register simplex k_x2 (rounds 1-4); 1: one-step plans (k_xq_thread, plan mode) streamed by k_x1, from the generating parent only; 2 (default): ... and from the candidate's other parents
    long long xqt_min = 4096, x1_min = 2048;   // MPC_XQT_MIN / MPC_X1_MIN: smallest list the one-thread pass / the one-step plans take (tests set 1: every level of a small program goes through them)
    int x1_wpc = 16;          // MPC_X1_WPC: wavefronts per CU of k_x1 (config 4, level 4, beside the region kernel: x stage 1.13 / 0.95 / 1.02 ms with 8 / 16 / 32)
    long long xq_early_regions = 0;   // MPC_XQ_EARLY_REGIONS = r > 0: the pass runs beside the theta stage only when the level before found fewer than r regions (0: always)
    int xqt_wpc = 16;         // MPC_XQT_WPC: wavefronts per CU of k_xq_thread (it is bound by the cache's request rate: config 4's level 0.45 ms alone with 8 per CU, 0.49 with 24; beside the region kernel 0.92 / 0.70 / 0.78 / 0.75 with 4 / 8 / 12 / 16)
    int xq_thread = -1;       // MPC_XQ_THREAD: 0 = the quick test without its one-thread-per-candidate first pass k_xq_thread (round 5); 1 = the pass against the generating parent only; n >= 2 = ... and up to n - 1 other parents; default: every other parent
    int no_kkt_thread = 0;    // MPC_NO_KKT_THREAD=1: KKT solves stay inside the wave kernels (A/B); 2: only the small-level path
    int force_v1 = 0;         // MPC_FORCE_V1=1 in the environment: never use k_verdict2 (A/B comparisons, tests)
    double dict_budget_gb = 48.0;   // MPC_DICT_BUDGET_GB: device memory both generations of the (x,theta) dictionary cache may hold
    // ---- read by creation alone (create.hpp) -------------------------------------------------------------------------------------------
    bool no_eq_elim = false;  // MPC_NO_EQ_ELIM=1: the equality rows are not eliminated from the Schur blocks (setup_mfma.hpp; tests)
    bool kkt_box_select = false;   // MPC_KKT_BOX_SELECT=1: the select form of the screen's row test on every program (tests)
    int th_div = 4;           // MPC_TH_DIV: work items per wavefront of k_theta2 (<= 0 = round-3 behaviour: where targs is filled it zeroes wave_div and wave_max)
    int th_maxw = 2;          // MPC_TH_MAXW: waves per SIMD of k_theta2 (x 4 x n_cu where targs is filled)
    bool debug_create = false;   // MPC_DEBUG_CREATE set (any value): the decisions of creation on stderr

    static Knobs from_env();
};

// how a row's value is read from the text of its variable
enum class KnobKind {
    flag,         // true iff set and the first character is '1'
    present,      // true iff set, even when empty
    integer,      // atoi when set, else the default
    int_ge0,      // max(0, atoi) when set
    int_gt0,      // taken only when atoi > 0
    pct_gt0,      // ... and then at most 100
    int64,        // atoll when set
    real,         // atof when set
    rsplit,       // atoi rounded down to one of 16, 8, 4, 2, 1 (anything below 2 gives 1)
    int_nonempty  // atoi when set and not empty (process-wide rows: the shares of the shared launches)
};
enum class KnobWhen { handle, process, call };   // read at every mpc_create / once per process / at every call of the entry point named in the row

struct KnobRow {
    const char *name;
    KnobKind kind;
    KnobWhen when;
    const char *what;
    int Knobs::*pi = nullptr;            // the member the value goes to: exactly one of the four, none for a process-wide row
    bool Knobs::*pb = nullptr;
    long long Knobs::*pl = nullptr;
    double Knobs::*pd = nullptr;
    double dflt = 0.0;                   // default of a process-wide row (a handle row's default is its member's initialiser)
    constexpr KnobRow(const char *n, KnobKind k, int Knobs::*m, const char *w) : name(n), kind(k), when(KnobWhen::handle), what(w), pi(m) {}
    constexpr KnobRow(const char *n, KnobKind k, bool Knobs::*m, const char *w) : name(n), kind(k), when(KnobWhen::handle), what(w), pb(m) {}
    constexpr KnobRow(const char *n, KnobKind k, long long Knobs::*m, const char *w) : name(n), kind(k), when(KnobWhen::handle), what(w), pl(m) {}
    constexpr KnobRow(const char *n, KnobKind k, double Knobs::*m, const char *w) : name(n), kind(k), when(KnobWhen::handle), what(w), pd(m) {}
    constexpr KnobRow(const char *n, KnobKind k, KnobWhen wh, double d, const char *w) : name(n), kind(k), when(wh), what(w), dflt(d) {}
};

inline constexpr KnobRow KNOB_TABLE[] = {
    // ---- per handle: Knobs::from_env() at mpc_create ---------------------------------------------------------------------------------
    {"MPC_FORCE_V1", KnobKind::flag, &Knobs::force_v1, "LDS-engine kernels only: never k_verdict2"},
    {"MPC_DEBUG_CYCLES", KnobKind::flag, &Knobs::debug_cycles, "per-level cycle breakdown on stderr"},
    {"MPC_NO_RSPLIT", KnobKind::flag, &Knobs::no_rsplit, "one wavefront per candidate in k_region2"},
    {"MPC_NO_RBOX", KnobKind::flag, &Knobs::no_rbox, "no bounding-box screen of the region rows in k_region2"},
    {"MPC_NO_ROVERLAP", KnobKind::flag, &Knobs::no_roverlap, "region stage behind, not beside, the (x,theta) stage"},
    {"MPC_NO_KKT_LISTS", KnobKind::flag, &Knobs::no_kkt_lists, "work lists behind k_kkt_thread by compaction of the status array"},
    {"MPC_NO_SMALL_RX", KnobKind::flag, &Knobs::no_small_rx, "region and (x,theta) kernel of a small level as two launches"},
    {"MPC_NO_SMALL_FUSE", KnobKind::flag, &Knobs::no_small_fuse, "the small path with its round-4 launches"},
    {"MPC_NO_SMALLPATH", KnobKind::flag, &Knobs::no_smallpath, "every level on the classic path with its host round trips"},
    {"MPC_TEST_SMALL_FALLBACK", KnobKind::flag, &Knobs::test_small_fallback, "tests: every small level reports 'repeat on the classic path'"},
    {"MPC_NO_EQ_ELIM", KnobKind::flag, &Knobs::no_eq_elim, "equality rows not eliminated from the Schur blocks"},
    {"MPC_KKT_BOX_SELECT", KnobKind::flag, &Knobs::kkt_box_select, "k_kkt_thread's row test over the bounding box with selects"},
    {"MPC_DEBUG_CREATE", KnobKind::present, &Knobs::debug_create, "the decisions of creation on stderr"},
    {"MPC_X1_DEFER", KnobKind::integer, &Knobs::x1_defer, "k_x1 on its own stream beside the end of its level; 0: in line"},
    {"MPC_KKT_SPREAD", KnobKind::integer, &Knobs::kkt_spread, "eight lanes per candidate in k_kkt_thread on small levels; 0: one lane"},
    {"MPC_XQ_THREAD", KnobKind::integer, &Knobs::xq_thread, "quick test's one-thread pass: 0 off, 1 generating parent only, n >= 2 up to n - 1 other parents, -1 all"},
    {"MPC_X1", KnobKind::integer, &Knobs::x1, "one-step plans on storing levels: 0 k_x2 only, 1 generating parent only, 2 other parents too"},
    {"MPC_NO_KKT_THREAD", KnobKind::integer, &Knobs::no_kkt_thread, "1: KKT solves inside the wave kernels; 2: only on the small-level path"},
    {"MPC_TEST_LATE", KnobKind::integer, &Knobs::test_late, "tests: the overlapped launch leaves N optimal candidates to the late path"},
    {"MPC_TEST_SPARE", KnobKind::integer, &Knobs::test_spare, "tests: N fewer spare region slots behind the overlapped launch"},
    {"MPC_TH_DIV", KnobKind::integer, &Knobs::th_div, "work items per wavefront of k_theta2; <= 0: one wavefront per item"},
    {"MPC_TH_MAXW", KnobKind::integer, &Knobs::th_maxw, "most waves per SIMD of k_theta2"},
    {"MPC_KKT_SPREAD_THREADS", KnobKind::int_ge0, &Knobs::kkt_spread_threads, "classic path: most threads of the spread form of k_kkt_thread"},
    {"MPC_X_SECOND_MAX", KnobKind::int_ge0, &Knobs::x_second_max, "k_x2: a level's budget of doubtful cached runs repeated from D0; 0: all go to the LDS engine"},
    {"MPC_XQ_SKIP_BELOW", KnobKind::int_ge0, &Knobs::xq_skip_below, "the last level's quick test leaves a shorter list to k_x2; 0: never"},
    {"MPC_XQT_WPC", KnobKind::int_gt0, &Knobs::xqt_wpc, "wavefronts per CU of k_xq_thread"},
    {"MPC_X1_WPC", KnobKind::int_gt0, &Knobs::x1_wpc, "wavefronts per CU of k_x1"},
    {"MPC_X2_WPC", KnobKind::int_gt0, &Knobs::x2_wpc, "most wavefronts per CU of k_x2"},
    {"MPC_XQ_WPC", KnobKind::int_gt0, &Knobs::xq_wpc, "wavefronts per CU of k_xq"},
    {"MPC_XQG_PER_CU", KnobKind::int_gt0, &Knobs::xqg_per_cu, "workgroups per CU of k_xq_grouped"},
    {"MPC_X2_DIV", KnobKind::int_gt0, &Knobs::x2_div, "items per wavefront of k_x2"},
    {"MPC_R2_CAP", KnobKind::pct_gt0, &Knobs::r2_cap_pct, "per cent of k_region2's wave slots an overlapped launch may take"},
    {"MPC_PRUNED_BUCKET_NP", KnobKind::int64, &Knobs::pruned_bucket_np, "fewest pruned sets for which the pruned list is bucketed"},
    {"MPC_XQT_MIN", KnobKind::int64, &Knobs::xqt_min, "smallest list the quick test's one-thread pass takes"},
    {"MPC_X1_MIN", KnobKind::int64, &Knobs::x1_min, "smallest list the one-step plans take"},
    {"MPC_XQ_EARLY_REGIONS", KnobKind::int64, &Knobs::xq_early_regions, "r > 0: the one-thread pass beside the theta stage only after a level of fewer than r regions"},
    {"MPC_X_FIRST_MIN", KnobKind::int64, &Knobs::x_first_min, "smallest level whose (x,theta) stage is queued before the read-back"},
    {"MPC_X_FIRST_MAX", KnobKind::int64, &Knobs::x_first_max, "largest such level"},
    {"MPC_SMALLPATH_MAX", KnobKind::int64, &Knobs::smallpath_max, "largest level that runs without host round trips"},
    {"MPC_ROVERLAP_MIN", KnobKind::int64, &Knobs::roverlap_min, "fewest items of the (x,theta) stage beside which the region stage runs"},
    {"MPC_ROVERLAP_LONG", KnobKind::int64, &Knobs::roverlap_long, "items of the (x,theta) stage from which the overlapped region launch is capped"},
    {"MPC_X_FRESH_LIMIT", KnobKind::real, &Knobs::x_fresh_limit, "k_x2: growth up to which a run from D0 decides; 0: 1e3 as for cached runs"},
    {"MPC_PRUNED_BUCKET_MIN", KnobKind::real, &Knobs::pruned_bucket_min, "parents x pruned sets from which the pruned list is bucketed; 0: never"},
    {"MPC_DICT_BUDGET_GB", KnobKind::real, &Knobs::dict_budget_gb, "memory budget of the dictionary cache"},
    {"MPC_RSPLIT_MAX", KnobKind::rsplit, &Knobs::rsplit_max, "most wavefronts that share one optimal candidate in k_region2"},
    // ---- process-wide: knob_process(name), each at the moment named here ---------------------------------------------------------------
    {"MPC_DEV_POOL_GB", KnobKind::real, KnobWhen::process, 48.0, "free device blocks the pool keeps (read when the library is loaded)"},
    {"MPC_BATCH_WPC_TH", KnobKind::int_nonempty, KnobWhen::process, 32, "shared launches: wavefronts per CU of the theta kernel (the six shares are read at the first shared launch)"},
    {"MPC_BATCH_WPC_XQ", KnobKind::int_nonempty, KnobWhen::process, 20, "shared launches: wavefronts per CU of k_xq"},
    {"MPC_BATCH_WPC_X2", KnobKind::int_nonempty, KnobWhen::process, 12, "shared launches: wavefronts per CU of k_x2"},
    {"MPC_BATCH_WPC_R2", KnobKind::int_nonempty, KnobWhen::process, 16, "shared launches: wavefronts per CU of the region kernel"},
    {"MPC_BATCH_SHARES", KnobKind::int_nonempty, KnobWhen::process, 1, "shared launches: 0: every member the width of a single program's launch"},
    {"MPC_BATCH_WSHARE", KnobKind::int_nonempty, KnobWhen::process, 1, "shared launches: 0: a member's share does not bound the wavefronts per region"},
    {"MPC_BATCH_BUDGET_GB", KnobKind::real, KnobWhen::call, 160.0, "device memory the members of one shared launch may hold (read by every mpc_level_batch_start / mpc_solve_many)"},
    {"MPC_DEBUG_MANY", KnobKind::flag, KnobWhen::process, 0, "mpc_solve_many: per-level times and members outside the copy launch on stderr (read at the first of those)"},
    {"MPC_DEBUG_SMALL", KnobKind::flag, KnobWhen::process, 0, "small-path statistics on stderr at exit (read at the first small level)"},
};

// the value of row r given the text of its variable (nullptr: unset) and the value it has without it
inline double knob_parse(const KnobRow &r, const char *ev, double dflt) {
    switch (r.kind) {
        case KnobKind::flag: return ev && ev[0] == '1';
        case KnobKind::present: return ev != nullptr;
        case KnobKind::integer: return ev ? std::atoi(ev) : dflt;
        case KnobKind::int_ge0: return ev ? std::max(0, std::atoi(ev)) : dflt;
        case KnobKind::int_gt0: return ev && std::atoi(ev) > 0 ? std::atoi(ev) : dflt;
        case KnobKind::pct_gt0: return ev && std::atoi(ev) > 0 ? std::min(100, std::atoi(ev)) : dflt;
        case KnobKind::int64: return dflt;   // (64-bit values do not pass through a double: Knobs::from_env reads them itself)
        case KnobKind::real: return ev ? std::atof(ev) : dflt;
        case KnobKind::rsplit: { if (!ev) return dflt; const int v = std::atoi(ev); return v >= 16 ? 16 : (v >= 8 ? 8 : (v >= 4 ? 4 : (v >= 2 ? 2 : 1))); }
        case KnobKind::int_nonempty: return ev && *ev ? std::atoi(ev) : dflt;
    }
    return dflt;
}

inline Knobs Knobs::from_env() {
    Knobs k;
    for (const KnobRow &r : KNOB_TABLE) {
        if (r.when != KnobWhen::handle) continue;
        const char *ev = std::getenv(r.name);
        if (r.pl) { if (ev) k.*r.pl = std::atoll(ev); }
        else if (r.pd) k.*r.pd = knob_parse(r, ev, k.*r.pd);
        else if (r.pb) k.*r.pb = knob_parse(r, ev, k.*r.pb) != 0.0;
        else k.*r.pi = (int)knob_parse(r, ev, k.*r.pi);
    }
    return k;
}

// a process-wide row, read now
inline double knob_process(const char *name) {
    for (const KnobRow &r : KNOB_TABLE)
        if (r.when != KnobWhen::handle && std::strcmp(r.name, name) == 0) return knob_parse(r, std::getenv(r.name), r.dflt);
    std::abort();   // not a row of the table
}

}  // namespace
}  // namespace mpc
