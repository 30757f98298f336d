// vertices.hpp -- vertex enumeration of a batch of polytopes {theta : E theta <= f} (gfx950); DESIGN §3.16.
//
// One WORKGROUP per polytope runs the double-description method on the homogenised cone
//   {y = (theta, t) : f_r t - e_r theta >= 0 (r < m),  t >= 0 (row m)}
// whose extreme rays with t > 0 are the vertices (theta / t) and with t = 0 the rays of the polytope.
//   1. The m + 1 rows, scaled to unit 2-norm, are staged in LDS.  Complete-pivoting elimination picks n_t + 1 independent rows (the
//      basis); no such rows: the cone has a line (rank E < n_t), status NOT_POINTED.  The initial generators are the columns of the
//      basis matrix's inverse (Gauss-Jordan in LDS), scaled to unit 2-norm; generator j is tight on every basis row but row j.
//   2. The other rows are added one at a time in lexicographic order of their scaled coefficients (f first: "lexmin").  s_k = a_r . y_k
//      splits the generators into + (s > VX_EPS), 0 and -; row r joins the zero set Z of the 0 generators.  Without a - generator the
//      list stays.  Otherwise the next list is the + and 0 generators and, for every ADJACENT pair (u in +, v in -), the new generator
//      s_u y_v - s_v y_u (unit 2-norm) with Z = Z(u) & Z(v) | {r}.  Adjacency is combinatorial: |Z(u) & Z(v)| >= n_t - 1 and no third
//      generator w has Z(w) >= Z(u) & Z(v).  Z is a mask of VX_MW words (256 rows and the t row).
//   3. The lists live in a per-polytope slab of global memory, double-buffered ([2][cap] generators); new generators are compacted
//      through an LDS counter.  A list longer than cap ends the polytope with status OVERFLOW (the host repeats it with a larger slab).
//   4. The final generators: no generator, or a row of E tight at all of them (no interior) -> EMPTY.  Those without the t row in Z are
//      vertices theta = y / t, the others rays (unit 2-norm); rays make the status UNBOUNDED.  Vertices are sorted lexicographically
//      (rank sort), a vertex within tol (1 + |v|_inf) in every coordinate of a vertex before it in that order is dropped (a merge), and
//      the incidence of the survivors is recomputed from the unscaled rows: row r is tight when |f_r - e_r v| <= tol (1 + |f_r|).
//      Rays are sorted the same way, after the vertices in the slab.  k_vertices_gather packs the slabs into the outputs.
// The final order does not depend on the order of the compaction, so two runs give the same bits.
#pragma once
#include <stdint.h>

namespace mpc {

constexpr int VX_BLOCK = 256, VX_MAX_ROWS = 256, VX_MW = 5, VX_OUT_MW = 4;
constexpr int VX_OK = 0, VX_UNBOUNDED = 1, VX_NOT_POINTED = 2, VX_EMPTY = 3, VX_OVERFLOW = 4;
constexpr double VX_EPS = 1e-10;          // zero test of a_r . y: unit rows, unit generators
constexpr double VX_RANK_EPS = 1e-9;      // smallest pivot of the basis elimination

struct VxArgs {
    int nt;
    long long n;                  // polytopes in this launch
    const int32_t *poly;          // [n]: the polytope of workgroup q
    const long long *row_off;
    const double *ef;             // [rows][nt + 1] = [f | E]
    long long cap;                // generators per list
    double *slab_y;               // [n][2][cap][NT + 1]
    unsigned long long *slab_z;   // [n][2][cap][VX_MW]
    double *slab_s;               // [n][cap]
    int32_t *slab_i;              // [n][2][cap]
    double tol;
    int32_t *status, *n_vert, *n_ray, *buf;   // [n]; buf: the list that holds the results
    unsigned long long *counters;              // [n][3]: generators made, largest list, merges
};

// lexicographic order of two points of n coordinates (strided rows), ties broken by index
__device__ inline bool vx_before(const double *p, int i, const double *q, int j, int n) {
    for (int c = 0; c < n; ++c) {
        if (p[c] < q[c]) return true;
        if (p[c] > q[c]) return false;
    }
    return i < j;
}

template <int NT>
__global__ void __launch_bounds__(VX_BLOCK) k_region_vertices(VxArgs a) {
    constexpr int D = NT + 1, NW = VX_BLOCK / 64;
    __shared__ double R[VX_MAX_ROWS + 1][D];
    __shared__ double G[D][2 * D];
    __shared__ double fac[D];
    __shared__ int order[VX_MAX_ROWS + 1];
    __shared__ int used[VX_MAX_ROWS + 1];
    __shared__ int basis[D];
    __shared__ double red_v[NW];
    __shared__ int red_i[NW];
    __shared__ int cnt[4];
    __shared__ unsigned long long andz[VX_MW];
    const int tid = threadIdx.x;
    const long long q = blockIdx.x;
    const long long P = a.poly[q], r0 = a.row_off[P];
    const int m = (int)(a.row_off[P + 1] - r0), mh = m + 1, nt = a.nt, d = nt + 1;
    const long long cap = a.cap;
    double *Y0 = a.slab_y + q * 2 * cap * D;
    unsigned long long *Z0 = a.slab_z + q * 2 * cap * VX_MW;
    double *S = a.slab_s + q * cap;
    int32_t *PL = a.slab_i + q * 2 * cap, *MI = PL + cap;
    auto load_rows = [&]() {
        for (int r = tid; r < mh; r += VX_BLOCK) {
            if (r < m) {
                const double *row = a.ef + (r0 + r) * (nt + 1);
                double nn = 0.0;
                for (int c = 0; c <= nt; ++c) nn += row[c] * row[c];
                const double inv = nn > 0.0 ? 1.0 / sqrt(nn) : 1.0;
                for (int c = 0; c < nt; ++c) R[r][c] = -row[1 + c] * inv;
                R[r][nt] = row[0] * inv;
            } else {
                for (int c = 0; c < nt; ++c) R[r][c] = 0.0;
                R[r][nt] = 1.0;
            }
            used[r] = 0;
        }
    };
    auto finish = [&](int st, int nv, int nr, int b, unsigned long long made, unsigned long long largest, unsigned long long merges) {
        if (tid == 0) {
            a.status[q] = st; a.n_vert[q] = nv; a.n_ray[q] = nr; a.buf[q] = b;
            a.counters[q * 3 + 0] = made; a.counters[q * 3 + 1] = largest; a.counters[q * 3 + 2] = merges;
        }
    };
    load_rows();
    __syncthreads();
    // 1. the basis: complete pivoting on the scaled rows (R is overwritten, then staged again)
    unsigned colmask = 0;
    bool pointed = true;
    for (int s = 0; s < d; ++s) {
        double best = -1.0;
        int bi = 0x7fffffff;
        for (int r = tid; r < mh; r += VX_BLOCK) {
            if (used[r]) continue;
            for (int c = 0; c < d; ++c) {
                if ((colmask >> c) & 1u) continue;
                const double v = fabs(R[r][c]);
                const int id = r * D + c;
                if (v > best || (v == best && id < bi)) { best = v; bi = id; }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best, off);
            const int oi = __shfl_xor(bi, off);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if ((tid & 63) == 0) { red_v[tid >> 6] = best; red_i[tid >> 6] = bi; }
        __syncthreads();
        best = red_v[0]; bi = red_i[0];
        for (int w = 1; w < NW; ++w)
            if (red_v[w] > best || (red_v[w] == best && red_i[w] < bi)) { best = red_v[w]; bi = red_i[w]; }
        __syncthreads();
        if (!(best > VX_RANK_EPS)) { pointed = false; break; }
        const int pr = bi / D, pc = bi % D;
        colmask |= 1u << pc;
        if (tid == 0) { basis[s] = pr; used[pr] = 1; }
        __syncthreads();
        const double pv = R[pr][pc];
        for (int r = tid; r < mh; r += VX_BLOCK) {
            if (used[r]) continue;
            const double f = R[r][pc] / pv;
            for (int c = 0; c < d; ++c) R[r][c] -= f * R[pr][c];
        }
        __syncthreads();
    }
    if (!pointed) { finish(VX_NOT_POINTED, 0, 0, 0, 0, 0, 0); return; }
    // stage the rows again (used[] is reset too: mark the basis once more)
    load_rows();
    __syncthreads();
    if (tid < d) used[basis[tid]] = 1;
    // G = [A_basis | I], Gauss-Jordan with partial pivoting
    for (int idx = tid; idx < d * 2 * d; idx += VX_BLOCK) {
        const int i = idx / (2 * d), j = idx % (2 * d);
        G[i][j] = j < d ? R[basis[i]][j] : (j - d == i ? 1.0 : 0.0);
    }
    __syncthreads();
    for (int c = 0; c < d; ++c) {
        if (tid == 0) {
            int p = c;
            for (int r = c + 1; r < d; ++r) if (fabs(G[r][c]) > fabs(G[p][c])) p = r;
            if (p != c)
                for (int j = 0; j < 2 * d; ++j) { const double t = G[p][j]; G[p][j] = G[c][j]; G[c][j] = t; }
        }
        __syncthreads();
        if (tid < d) fac[tid] = G[tid][c] / G[c][c];
        __syncthreads();
        for (int idx = tid; idx < d * 2 * d; idx += VX_BLOCK) {
            const int i = idx / (2 * d), j = idx % (2 * d);
            if (i != c) G[i][j] -= fac[i] * G[c][j];
        }
        __syncthreads();
    }
    if (tid < d) fac[tid] = G[tid][tid];
    __syncthreads();
    // generator j: column j of the inverse (row swaps permute the rows of G, not the columns of the inverse)
    if (tid < d) {
        const int j = tid;
        double nn = 0.0;
        for (int i = 0; i < d; ++i) { const double v = G[i][d + j] / fac[i]; nn += v * v; }
        const double inv = 1.0 / sqrt(nn);
        for (int i = 0; i < d; ++i) Y0[(long long)j * D + i] = G[i][d + j] / fac[i] * inv;
        for (int w = 0; w < VX_MW; ++w) Z0[(long long)j * VX_MW + w] = 0ull;
        for (int k = 0; k < d; ++k)
            if (k != j) Z0[(long long)j * VX_MW + (basis[k] >> 6)] |= 1ull << (basis[k] & 63);
    }
    // the other rows in lexmin order: f first, then -e (rank sort)
    for (int r = tid; r < mh; r += VX_BLOCK) {
        if (used[r]) continue;
        int rank = 0;
        for (int o = 0; o < mh; ++o) {
            if (used[o] || o == r) continue;
            bool before = false, decided = false;
            if (R[o][nt] != R[r][nt]) { before = R[o][nt] < R[r][nt]; decided = true; }
            for (int c = 0; c < nt && !decided; ++c)
                if (R[o][c] != R[r][c]) { before = R[o][c] < R[r][c]; decided = true; }
            if (!decided) before = o < r;
            rank += before;
        }
        order[rank] = r;
    }
    __syncthreads();
    // 2. the double description
    long long N = d;
    int cur = 0;
    unsigned long long largest = d, made = d;
    bool overflow = false;
    if (tid == 0) cnt[3] = 0;
    for (int k = 0; k < mh - d; ++k) {
        const int r = order[k];
        double *Yc = Y0 + (long long)cur * cap * D, *Yn = Y0 + (long long)(cur ^ 1) * cap * D;
        unsigned long long *Zc = Z0 + (long long)cur * cap * VX_MW, *Zn = Z0 + (long long)(cur ^ 1) * cap * VX_MW;
        if (tid == 0) { cnt[0] = 0; cnt[1] = 0; cnt[2] = 0; }
        __syncthreads();
        for (long long g = tid; g < N; g += VX_BLOCK) {
            double s = 0.0;
            for (int c = 0; c < d; ++c) s += R[r][c] * Yc[g * D + c];
            S[g] = s;
            if (s > VX_EPS) PL[atomicAdd(&cnt[0], 1)] = (int32_t)g;
            else if (s < -VX_EPS) MI[atomicAdd(&cnt[1], 1)] = (int32_t)g;
            else Zc[g * VX_MW + (r >> 6)] |= 1ull << (r & 63);
        }
        __syncthreads();
        const long long np = cnt[0], nm = cnt[1];
        __syncthreads();
        if (nm == 0) continue;
        for (long long g = tid; g < N; g += VX_BLOCK) {
            if (!(S[g] >= -VX_EPS)) continue;
            const long long pos = atomicAdd(&cnt[2], 1);
            if (pos >= cap) continue;
            for (int c = 0; c < d; ++c) Yn[pos * D + c] = Yc[g * D + c];
#pragma unroll
            for (int w = 0; w < VX_MW; ++w) Zn[pos * VX_MW + w] = Zc[g * VX_MW + w];
        }
        const long long npairs = np * nm;
        for (long long p = tid; p < npairs; p += VX_BLOCK) {
            const long long u = PL[p / nm], v = MI[p % nm];
            unsigned long long C[VX_MW];
            int pc = 0;
#pragma unroll
            for (int w = 0; w < VX_MW; ++w) { C[w] = Zc[u * VX_MW + w] & Zc[v * VX_MW + w]; pc += __popcll(C[w]); }
            if (pc < d - 2) continue;
            bool adj = true;
            for (long long g = 0; g < N && adj; ++g) {
                if (g == u || g == v) continue;
                bool sup = true;
#pragma unroll
                for (int w = 0; w < VX_MW; ++w) sup = sup && (Zc[g * VX_MW + w] & C[w]) == C[w];
                adj = !sup;
            }
            if (!adj) continue;
            const double su = S[u], sv = S[v];
            double nn = 0.0;
            for (int c = 0; c < d; ++c) { const double y = su * Yc[v * D + c] - sv * Yc[u * D + c]; nn += y * y; }
            const double inv = 1.0 / sqrt(nn);
            const long long pos = atomicAdd(&cnt[2], 1);
            atomicAdd(&cnt[3], 1);
            if (pos >= cap) continue;
            for (int c = 0; c < d; ++c) Yn[pos * D + c] = (su * Yc[v * D + c] - sv * Yc[u * D + c]) * inv;
#pragma unroll
            for (int w = 0; w < VX_MW; ++w) Zn[pos * VX_MW + w] = w == (r >> 6) ? C[w] | 1ull << (r & 63) : C[w];
        }
        __syncthreads();
        const long long nn = cnt[2];
        __syncthreads();
        if (nn > cap) { overflow = true; N = nn; break; }
        N = nn;
        cur ^= 1;
        largest = N > (long long)largest ? (unsigned long long)N : largest;
    }
    made += (unsigned long long)cnt[3];
    if (overflow) { finish(VX_OVERFLOW, 0, 0, 0, made, N, 0); return; }
    // 3. the final generators: interior, vertices and rays
    double *Yc = Y0 + (long long)cur * cap * D, *Yn = Y0 + (long long)(cur ^ 1) * cap * D;
    unsigned long long *Zc = Z0 + (long long)cur * cap * VX_MW, *Zn = Z0 + (long long)(cur ^ 1) * cap * VX_MW;
    if (tid < VX_MW) andz[tid] = ~0ull;
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; cnt[2] = 0; }
    __syncthreads();
    for (long long g = tid; g < N; g += VX_BLOCK)
#pragma unroll
        for (int w = 0; w < VX_MW; ++w) atomicAnd(&andz[w], Zc[g * VX_MW + w]);
    __syncthreads();
    bool interior = N > 0;
#pragma unroll
    for (int w = 0; w < VX_MW; ++w) {
        unsigned long long bits = andz[w];
        if (w == (m >> 6)) bits &= (1ull << (m & 63)) - 1ull;    // rows of E only: not the t row
        if (w > (m >> 6)) bits = 0ull;
        interior = interior && bits == 0ull;
    }
    if (!interior) { finish(VX_EMPTY, 0, 0, 0, made, largest, 0); return; }
    for (long long g = tid; g < N; g += VX_BLOCK) {
        const bool ray = (Zc[g * VX_MW + (m >> 6)] >> (m & 63)) & 1ull;
        if (!ray) {
            const long long pos = atomicAdd(&cnt[0], 1);
            const double t = Yc[g * D + nt];
            for (int c = 0; c < nt; ++c) Yn[pos * D + c] = Yc[g * D + c] / t;
        } else {
            const long long pos = cap - 1 - atomicAdd(&cnt[1], 1);
            double nn = 0.0;
            for (int c = 0; c < nt; ++c) nn += Yc[g * D + c] * Yc[g * D + c];
            const double inv = 1.0 / sqrt(nn);
            for (int c = 0; c < nt; ++c) Yn[pos * D + c] = Yc[g * D + c] * inv;
        }
    }
    __syncthreads();
    const long long V = cnt[0], NR = cnt[1];
    if (V == 0) { finish(VX_EMPTY, 0, 0, 0, made, largest, 0); return; }
    // ranks (PL), then the merge flags (S), then the survivors' places
    for (long long i = tid; i < V; i += VX_BLOCK) {
        int rank = 0;
        for (long long j = 0; j < V; ++j) rank += j != i && vx_before(Yn + j * D, (int)j, Yn + i * D, (int)i, nt);
        PL[i] = rank;
    }
    for (long long i = tid; i < NR; i += VX_BLOCK) {
        const long long pi = cap - 1 - i;
        int rank = 0;
        for (long long j = 0; j < NR; ++j) rank += j != i && vx_before(Yn + (cap - 1 - j) * D, (int)j, Yn + pi * D, (int)i, nt);
        MI[i] = rank;
    }
    __syncthreads();
    for (long long i = tid; i < V; i += VX_BLOCK) {
        double sc = 0.0;
        for (int c = 0; c < nt; ++c) sc = fmax(sc, fabs(Yn[i * D + c]));
        const double lim = a.tol * (1.0 + sc);
        bool drop = false;
        for (long long j = 0; j < V && !drop; ++j) {
            if (PL[j] >= PL[i]) continue;
            bool close = true;
            for (int c = 0; c < nt && close; ++c) close = fabs(Yn[j * D + c] - Yn[i * D + c]) <= lim;
            drop = close;
        }
        S[i] = drop ? 1.0 : 0.0;
    }
    __syncthreads();
    for (long long i = tid; i < V; i += VX_BLOCK) {
        if (S[i] != 0.0) { atomicAdd(&cnt[2], 1); continue; }
        long long pos = 0;
        for (long long j = 0; j < V; ++j) pos += S[j] == 0.0 && PL[j] < PL[i];
        unsigned long long z[VX_OUT_MW] = {0ull, 0ull, 0ull, 0ull};
        for (int rr = 0; rr < m; ++rr) {
            const double *row = a.ef + (r0 + rr) * (nt + 1);
            double v = 0.0;
            for (int c = 0; c < nt; ++c) v += row[1 + c] * Yn[i * D + c];
            if (fabs(row[0] - v) <= a.tol * (1.0 + fabs(row[0]))) {
#pragma unroll
                for (int w = 0; w < VX_OUT_MW; ++w) if (w == (rr >> 6)) z[w] |= 1ull << (rr & 63);
            }
        }
        for (int c = 0; c < nt; ++c) Yc[pos * D + c] = Yn[i * D + c];
#pragma unroll
        for (int w = 0; w < VX_OUT_MW; ++w) Zc[pos * VX_MW + w] = z[w];
    }
    __syncthreads();
    const long long VK = V - cnt[2];
    for (long long i = tid; i < NR; i += VX_BLOCK)
        for (int c = 0; c < nt; ++c) Yc[(VK + MI[i]) * D + c] = Yn[(cap - 1 - i) * D + c];
    finish(NR > 0 ? VX_UNBOUNDED : VX_OK, (int)VK, (int)NR, cur, made, largest, (unsigned long long)cnt[2]);
}

// packs the results of every polytope of a launch: vertices, their incidence (VX_OUT_MW words) and rays at the host-given offsets
template <int NT>
__global__ void __launch_bounds__(VX_BLOCK) k_vertices_gather(int nt, long long cap, const double *slab_y, const unsigned long long *slab_z,
                                                               const int32_t *n_vert, const int32_t *n_ray, const int32_t *buf,
                                                               const long long *v_off, const long long *r_off, double *vert,
                                                               unsigned long long *inc, double *rays) {
    constexpr int D = NT + 1;
    const long long q = blockIdx.x;
    const double *Y = slab_y + (q * 2 + buf[q]) * cap * D;
    const unsigned long long *Z = slab_z + (q * 2 + buf[q]) * cap * VX_MW;
    const long long nv = n_vert[q], nr = n_ray[q], vo = v_off[q], ro = r_off[q];
    for (long long i = threadIdx.x; i < nv * nt; i += VX_BLOCK) vert[vo * nt + i] = Y[(i / nt) * D + i % nt];
    for (long long i = threadIdx.x; i < nv * VX_OUT_MW; i += VX_BLOCK) inc[vo * VX_OUT_MW + i] = Z[(i / VX_OUT_MW) * VX_MW + i % VX_OUT_MW];
    for (long long i = threadIdx.x; i < nr * nt; i += VX_BLOCK) rays[ro * nt + i] = Y[(nv + i / nt) * D + i % nt];
}

}  // namespace mpc
