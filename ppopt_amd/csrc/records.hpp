// records.hpp -- the layout of a region record, once: the fixed-stride record of include/mpcombi.h (mpc_level_regions) and the slot
// (compact) form the device writes (mpc_level_regions_compact), their sizes, the offsets of every block, and the conversions between the
// two on the host.  Plain C++ without a HIP include: MPC_HD is __host__ __device__ under hipcc and empty for a host compiler, which can
// build the header alone (tests/test_records_cpu.py).  The device merge (k_rretry_merge) and the fetch family (level_fetch.hpp) take every
// offset and head word from here; the writers (k_region, k_region2) and the facet readers (graph.hpp) take the head words and sum the
// list offsets from their own arguments, with a comment naming the member here that each sum equals.
//
//   fixed:  rec_d doubles  A_x[nx*nt] b_x[nx] | A_l[nc*nt] | b_l[nc] | E[(nc+ntc)*nt] | f[nc+ntc]
//           rec_i ints     k nE n_om n_la n_re | active[nc] | omega[ntc] | lambda[nc] | regular_idx[nc] | regular_con[nc]
//   slot:   fd doubles     A_x[nx*nt] b_x[nx] | A_l[k*nt] | b_l[k]
//           fi ints        status cand nE n_om n_la n_re row0 reason | active[k] | omega[ntc] | lambda[k] | regular_idx[nc-k] | regular_con[nc-k]
//           row pool       row_len = nt+1 doubles per row: f, E[0..nt); a region owns rows row0 .. row0+nE-1
//   unused entries: -1 in ints, 0.0 in doubles
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPC_HD __host__ __device__
#else
#define MPC_HD
#endif

namespace mpc {

// head words of a slot's ints / of a fixed record's ints (the lists follow)
enum SlotWord { SW_STATUS, SW_CAND, SW_NE, SW_NOM, SW_NLA, SW_NRE, SW_ROW0, SW_REASON, SW_LISTS = 8 };
enum FixedWord { FW_K, FW_NE, FW_NOM, FW_NLA, FW_NRE, FW_LISTS = 5 };
constexpr int SLOT_ST_REGION = 3;   // MPC_REGION (mpcombi.h) = ST_REGION (kernels.hpp): the only status whose slot carries a record

struct RecordShape {
    int nx, nt, nc, ntc, neq, k;
    MPC_HD int row_len() const { return nt + 1; }
    MPC_HD int rows_t() const { return nc - neq + ntc; }    // rows a region can keep
    MPC_HD int law() const { return nx * nt + nx; }         // A_x | b_x: first in both forms
    MPC_HD int fd() const { return nx * nt + nx + k * nt + k; }
    MPC_HD int fi() const { return SW_LISTS + k + ntc + k + 2 * (nc - k); }
    MPC_HD long long rec_d() const { return (long long)nx * nt + nx + (long long)nc * nt + nc + (long long)(nc + ntc) * nt + (nc + ntc); }
    MPC_HD long long rec_i() const { return FW_LISTS + 4LL * nc + ntc; }
    // slot doubles
    MPC_HD int s_law() const { return 0; }
    MPC_HD int s_Al() const { return nx * nt + nx; }
    MPC_HD int s_bl() const { return nx * nt + nx + k * nt; }
    // slot ints
    MPC_HD int s_act() const { return SW_LISTS; }
    MPC_HD int s_om() const { return SW_LISTS + k; }
    MPC_HD int s_la() const { return SW_LISTS + k + ntc; }
    MPC_HD int s_ridx() const { return SW_LISTS + k + ntc + k; }
    MPC_HD int s_rcon() const { return SW_LISTS + k + ntc + k + (nc - k); }
    // fixed doubles
    MPC_HD int f_law() const { return 0; }
    MPC_HD int f_Al() const { return nx * nt + nx; }
    MPC_HD int f_bl() const { return nx * nt + nx + nc * nt; }
    MPC_HD int f_E() const { return nx * nt + nx + nc * nt + nc; }
    MPC_HD int f_f() const { return nx * nt + nx + nc * nt + nc + (nc + ntc) * nt; }
    // fixed int lists
    MPC_HD int f_act() const { return FW_LISTS; }
    MPC_HD int f_om() const { return FW_LISTS + nc; }
    MPC_HD int f_la() const { return FW_LISTS + nc + ntc; }
    MPC_HD int f_ridx() const { return FW_LISTS + nc + ntc + nc; }
    MPC_HD int f_rcon() const { return FW_LISTS + nc + ntc + nc + nc; }
};

// upper bound of the rows a level's records own: the pooled rows (k_region2) plus rows_t per candidate re-solved into a fixed record, or
// rows_t per region when nothing is pooled
MPC_HD inline long long record_rows_bound(const RecordShape &s, bool used_region2, long long n_erows, long long n_rretry, long long n_regions) {
    return used_region2 ? n_erows + n_rretry * s.rows_t() : n_regions * s.rows_t();
}

// Fixed record (rd, ri) -> slot (od, oi) with its rows [f | E] in erows from row0 on.  The slot's ints are always written (status, cand,
// zero counts, -1 lists); without a record (rd == nullptr) or with another status than a region's that is all.  Returns the rows written.
inline int fixed_to_slot(const RecordShape &s, const double *rd, const int32_t *ri, int status, int cand, long long row0, double *od, int32_t *oi, double *erows) {
    const int fi = s.fi(), fd = s.fd();
    for (int i = 0; i < fi; ++i) oi[i] = i < SW_LISTS ? 0 : -1;
    oi[SW_STATUS] = status; oi[SW_CAND] = cand;
    if (!rd || !ri || status != SLOT_ST_REGION) return 0;
    const int kk = ri[FW_K], nE = ri[FW_NE], n_om = ri[FW_NOM], n_la = ri[FW_NLA], n_re = ri[FW_NRE], nt = s.nt, nr = s.row_len();
    for (int i = 0; i < fd; ++i) od[i] = 0.0;
    for (int i = 0; i < s.law(); ++i) od[s.s_law() + i] = rd[s.f_law() + i];
    for (int i = 0; i < kk * nt; ++i) od[s.s_Al() + i] = rd[s.f_Al() + i];
    for (int i = 0; i < kk; ++i) od[s.s_bl() + i] = rd[s.f_bl() + i];
    oi[SW_NE] = nE; oi[SW_NOM] = n_om; oi[SW_NLA] = n_la; oi[SW_NRE] = n_re; oi[SW_ROW0] = (int32_t)row0;
    for (int i = 0; i < kk; ++i) oi[s.s_act() + i] = ri[s.f_act() + i];
    for (int i = 0; i < n_om; ++i) oi[s.s_om() + i] = ri[s.f_om() + i];
    for (int i = 0; i < n_la; ++i) oi[s.s_la() + i] = ri[s.f_la() + i];
    for (int i = 0; i < n_re; ++i) { oi[s.s_ridx() + i] = ri[s.f_ridx() + i]; oi[s.s_rcon() + i] = ri[s.f_rcon() + i]; }
    const double *E = rd + s.f_E(), *f = rd + s.f_f();
    for (int r = 0; r < nE; ++r) {
        double *row = erows + (size_t)(row0 + r) * nr;
        row[0] = f[r];
        for (int t = 0; t < nt; ++t) row[1 + t] = E[(size_t)r * nt + t];
    }
    return nE;
}

// Slot of a region (sd, si) with its rows in erows -> fixed record (rd, ri): the inverse.
inline void slot_to_fixed(const RecordShape &s, const double *sd, const int32_t *si, const double *erows, double *rd, int32_t *ri) {
    const long long rec_d = s.rec_d(), rec_i = s.rec_i();
    const int k = s.k, nt = s.nt, nr = s.row_len(), nE = si[SW_NE], n_om = si[SW_NOM], n_la = si[SW_NLA], n_re = si[SW_NRE];
    for (long long i = 0; i < rec_d; ++i) rd[i] = 0.0;
    for (long long i = 0; i < rec_i; ++i) ri[i] = -1;
    for (int i = 0; i < s.law(); ++i) rd[s.f_law() + i] = sd[s.s_law() + i];
    for (int i = 0; i < k * nt; ++i) rd[s.f_Al() + i] = sd[s.s_Al() + i];
    for (int i = 0; i < k; ++i) rd[s.f_bl() + i] = sd[s.s_bl() + i];
    double *E = rd + s.f_E(), *f = rd + s.f_f();
    for (int r = 0; r < nE; ++r) {
        const double *row = erows + (size_t)(si[SW_ROW0] + r) * nr;
        f[r] = row[0];
        for (int t = 0; t < nt; ++t) E[(size_t)r * nt + t] = row[1 + t];
    }
    ri[FW_K] = k; ri[FW_NE] = nE; ri[FW_NOM] = n_om; ri[FW_NLA] = n_la; ri[FW_NRE] = n_re;
    for (int i = 0; i < k; ++i) ri[s.f_act() + i] = si[s.s_act() + i];
    for (int i = 0; i < n_om; ++i) ri[s.f_om() + i] = si[s.s_om() + i];
    for (int i = 0; i < n_la; ++i) ri[s.f_la() + i] = si[s.s_la() + i];
    for (int i = 0; i < n_re; ++i) { ri[s.f_ridx() + i] = si[s.s_ridx() + i]; ri[s.f_rcon() + i] = si[s.s_rcon() + i]; }
}

}  // namespace mpc
