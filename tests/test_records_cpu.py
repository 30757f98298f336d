"""The layout of a region record (ppopt_amd/csrc/records.hpp): sizes, offsets and the two host conversions.  A tiny C++ program that
includes the header alone (g++, no HIP, built with the address and undefined-behaviour sanitizers) converts a fixed-stride record to the
slot form and back.  The fixed records are written here in numpy from the layout documented in include/mpcombi.h; the slot form is read
by RegionBatch and the fixed record by unpack_region -- two decoders the conversion shares no code with."""
import os
import shutil
import subprocess

import numpy
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'ppopt_amd', 'csrc')

MAIN = r'''
#include "records.hpp"
#include <cstdio>
#include <vector>
using namespace mpc;
// in:  int32 nx nt nc ntc neq k status cand row0 pool_rows used_region2 n_erows n_rretry n_regions, rec_d doubles, rec_i ints
// out: int64 fd fi rec_d rec_i rows_t row_len bound rows_written, slot doubles, slot ints, the row pool, the fixed record recovered
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t q[14];
    if (std::fread(q, 4, 14, in) != 14) return 3;
    const RecordShape s{q[0], q[1], q[2], q[3], q[4], q[5]};
    const int status = q[6], cand = q[7], row0 = q[8], pool_rows = q[9];
    std::vector<double> rd((size_t)s.rec_d()), od((size_t)s.fd(), 7.0), pool((size_t)pool_rows * s.row_len(), 9.0), rd2((size_t)s.rec_d(), 7.0);
    std::vector<int32_t> ri((size_t)s.rec_i()), oi((size_t)s.fi(), 7), ri2((size_t)s.rec_i(), 7);
    if (std::fread(rd.data(), 8, rd.size(), in) != rd.size() || std::fread(ri.data(), 4, ri.size(), in) != ri.size()) return 3;
    const int rows = fixed_to_slot(s, rd.data(), ri.data(), status, cand, row0, od.data(), oi.data(), pool.data());
    if (status == SLOT_ST_REGION) slot_to_fixed(s, od.data(), oi.data(), pool.data(), rd2.data(), ri2.data());
    const long long head[8] = {s.fd(), s.fi(), s.rec_d(), s.rec_i(), s.rows_t(), s.row_len(), record_rows_bound(s, q[10] != 0, q[11], q[12], q[13]), rows};
    std::fwrite(head, 8, 8, out);
    std::fwrite(od.data(), 8, od.size(), out); std::fwrite(oi.data(), 4, oi.size(), out); std::fwrite(pool.data(), 8, pool.size(), out);
    std::fwrite(rd2.data(), 8, rd2.size(), out); std::fwrite(ri2.data(), 4, ri2.size(), out);
    std::fclose(in); std::fclose(out);
    return 0;
}
'''

REGION = 3   # MPC_REGION


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ is needed to build the record converter')
    tmp = tmp_path_factory.mktemp('records')
    src, exe = str(tmp / 'main.cpp'), str(tmp / 'records')
    open(src, 'w').write(MAIN)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I', CSRC, src, '-o', exe])
    return exe, tmp


def fixed_record(rng, nx, nt, nc, ntc, k, nE, n_om, n_la, n_re):
    """One record in the layout of mpc_level_regions (include/mpcombi.h): unused entries 0.0 / -1."""
    A, b = rng.standard_normal((nx, nt)), rng.standard_normal(nx)
    Al, bl = numpy.zeros((nc, nt)), numpy.zeros(nc)
    Al[:k], bl[:k] = rng.standard_normal((k, nt)), rng.standard_normal(k)
    E, f = numpy.zeros((nc + ntc, nt)), numpy.zeros(nc + ntc)
    E[:nE], f[:nE] = rng.standard_normal((nE, nt)), rng.standard_normal(nE)
    rec_d = numpy.concatenate([A.ravel(), b, Al.ravel(), bl, E.ravel(), f])

    def padded(values, width):
        out = numpy.full(width, -1, dtype=numpy.int32)
        out[:len(values)] = values
        return out
    act = rng.choice(nc, size=k, replace=False)
    rec_i = numpy.concatenate([numpy.array([k, nE, n_om, n_la, n_re], dtype=numpy.int32), padded(act, nc),
                               padded(rng.choice(max(ntc, 1), size=n_om, replace=False), ntc), padded(rng.choice(nc, size=n_la, replace=False), nc),
                               padded(rng.choice(nc, size=n_re, replace=False), nc), padded(rng.choice(nc, size=n_re, replace=False), nc)])
    return numpy.ascontiguousarray(rec_d), numpy.ascontiguousarray(rec_i, dtype=numpy.int32)


def convert(program, shape, rec_d, rec_i, status=REGION, cand=11, row0=0, pool_rows=None, bound=(1, 0, 0, 0)):
    exe, tmp = program
    nx, nt, nc, ntc, neq, k = shape
    rows_t = nc - neq + ntc
    pool_rows = row0 + rows_t + 2 if pool_rows is None else pool_rows
    fin, fout = str(tmp / 'in.bin'), str(tmp / 'out.bin')
    with open(fin, 'wb') as fh:
        fh.write(numpy.array([nx, nt, nc, ntc, neq, k, status, cand, row0, pool_rows, *bound], dtype=numpy.int32).tobytes())
        fh.write(rec_d.tobytes())
        fh.write(rec_i.tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, 'rb').read()
    head = numpy.frombuffer(raw, dtype=numpy.int64, count=8)
    fd, fi, n_d, n_i = (int(v) for v in head[:4])
    o = 64
    od = numpy.frombuffer(raw, dtype=numpy.float64, count=fd, offset=o); o += 8 * fd
    oi = numpy.frombuffer(raw, dtype=numpy.int32, count=fi, offset=o); o += 4 * fi
    pool = numpy.frombuffer(raw, dtype=numpy.float64, count=pool_rows * (nt + 1), offset=o).reshape(pool_rows, nt + 1); o += 8 * pool_rows * (nt + 1)
    rd2 = numpy.frombuffer(raw, dtype=numpy.float64, count=n_d, offset=o); o += 8 * n_d
    ri2 = numpy.frombuffer(raw, dtype=numpy.int32, count=n_i, offset=o); o += 4 * n_i
    assert o == len(raw)
    return head, od, oi, pool, rd2, ri2


def check(program, rng, nx, nt, nc, ntc, neq, k, nE, n_om, n_la, n_re, row0=3):
    from ppopt_amd.mp_solvers.mpqp_hip_combinatorial import unpack_region
    from ppopt_amd.region_batch import RegionBatch
    shape = (nx, nt, nc, ntc, neq, k)
    rows_t = nc - neq + ntc
    assert k <= nc and nE <= rows_t and n_om <= ntc and n_la <= k and n_re <= nc - k
    rec_d, rec_i = fixed_record(rng, nx, nt, nc, ntc, k, nE, n_om, n_la, n_re)
    bound_in = (int(rng.integers(0, 2)), int(rng.integers(0, 50)), int(rng.integers(0, 5)), int(rng.integers(1, 9)))
    head, od, oi, pool, rd2, ri2 = convert(program, shape, rec_d, rec_i, cand=11, row0=row0, bound=bound_in)
    # sizes: the formulas of the host layer (Engine.slot_strides, Engine._rows_cap) and of mpcombi.h, as literals
    fd, fi = nx * nt + nx + k * nt + k, 8 + k + ntc + k + 2 * (nc - k)
    used, n_erows, n_rretry, n_regions = bound_in
    assert head.tolist() == [fd, fi, nx * nt + nx + nc * nt + nc + (nc + ntc) * nt + nc + ntc, 5 + 4 * nc + ntc, rows_t, nt + 1,
                             n_erows + n_rretry * rows_t if used else n_regions * rows_t, nE]
    assert (len(rec_d), len(rec_i)) == (head[2], head[3])
    # head words; the rows requested and no others
    assert oi[:8].tolist() == [REGION, 11, nE, n_om, n_la, n_re, row0, 0]
    untouched = numpy.ones(len(pool), dtype=bool)
    untouched[row0:row0 + nE] = False
    assert numpy.all(pool[untouched] == 9.0)
    # the same region through two independent decoders
    got = RegionBatch(od.reshape(1, fd), oi.reshape(1, fi), pool, nx, nt, nc, ntc, k).regions()[0]
    want = unpack_region(rec_d, rec_i, nx, nt, nc, ntc)
    for name in ('A', 'b', 'C', 'd', 'E', 'f'):
        a, w = getattr(got, name), getattr(want, name)
        assert a.shape == w.shape and numpy.array_equal(a, w), name
    for name in ('active_set', 'omega_set', 'lambda_set', 'regular_set'):
        assert getattr(got, name) == getattr(want, name), name
    # unused tails of the slot: -1 / 0.0
    o_la, o_ri = 8 + k + ntc, 8 + k + ntc + k
    o_rc = o_ri + nc - k
    assert numpy.all(oi[8 + k + n_om:o_la] == -1) and numpy.all(oi[o_la + n_la:o_ri] == -1)
    assert numpy.all(oi[o_ri + n_re:o_rc] == -1) and numpy.all(oi[o_rc + n_re:] == -1)
    assert not numpy.any(od == 7.0)
    # and back: bytewise
    assert rd2.tobytes() == rec_d.tobytes() and ri2.tobytes() == rec_i.tobytes()


EDGE_SHAPES = [
    # nx nt nc ntc neq k  nE n_om n_la n_re
    (3, 2, 6, 4, 0, 2, 5, 2, 1, 3),      # no equality rows
    (3, 2, 6, 4, 2, 2, 4, 1, 0, 2),      # the equality rows alone: n_eq = k
    (4, 3, 5, 6, 1, 5, 7, 3, 2, 0),      # k = n_c: regular_idx / regular_con have no entries
    (2, 2, 7, 0, 1, 3, 4, 0, 2, 4),      # n_tc = 0: an omega list of length zero
    (3, 2, 6, 3, 1, 2, 0, 0, 0, 0),      # nE = 0
    (3, 2, 6, 3, 1, 2, 8, 3, 1, 4),      # nE = rows_t
    (5, 1, 8, 2, 0, 3, 2, 1, 1, 0),      # one parameter
    (1, 1, 1, 0, 0, 0, 1, 0, 0, 1),      # the empty active set
]


@pytest.mark.parametrize('case', EDGE_SHAPES)
def test_edge_shapes(program, case):
    check(program, numpy.random.default_rng(5), *case)


def test_random_shapes(program):
    rng = numpy.random.default_rng(20)
    for _ in range(12):
        nx, nt, nc = int(rng.integers(1, 7)), int(rng.integers(1, 5)), int(rng.integers(1, 13))
        ntc = int(rng.integers(0, 2 * nt + 3))
        k = int(rng.integers(0, nc + 1))
        neq = int(rng.integers(0, k + 1))
        rows_t = nc - neq + ntc
        check(program, rng, nx, nt, nc, ntc, neq, k, int(rng.integers(0, rows_t + 1)), int(rng.integers(0, ntc + 1)), int(rng.integers(0, k + 1)),
              int(rng.integers(0, nc - k + 1)), row0=int(rng.integers(0, 6)))


def test_a_record_of_fewer_active_rows_leaves_the_slot_tails_unused(program):
    """The level kernels write records of exactly k active rows, so above every double of a slot is in use.  A record that names fewer
    (FW_K = k - 2) shows the fills of the slot's own tails: 0.0 in A_lambda / b_lambda, -1 in the active list."""
    nx, nt, nc, ntc, neq, k, kk = 3, 2, 6, 3, 0, 4, 2
    rec_d, rec_i = fixed_record(numpy.random.default_rng(2), nx, nt, nc, ntc, kk, 4, 1, 2, 2)
    assert rec_i[0] == kk
    head, od, oi, pool, _, _ = convert(program, (nx, nt, nc, ntc, neq, k), rec_d, rec_i, cand=5, row0=1)
    law = nx * nt + nx
    Al, bl = od[law:law + k * nt].reshape(k, nt), od[law + k * nt:]
    assert len(bl) == k and oi[:8].tolist() == [REGION, 5, 4, 1, 2, 2, 1, 0]
    assert numpy.array_equal(od[:law], rec_d[:law])
    assert numpy.array_equal(Al[:kk].ravel(), rec_d[law:law + kk * nt]) and numpy.array_equal(bl[:kk], rec_d[law + nc * nt:law + nc * nt + kk])
    assert numpy.all(Al[kk:] == 0.0) and numpy.all(bl[kk:] == 0.0)
    assert numpy.array_equal(oi[8:8 + kk], rec_i[5:5 + kk]) and numpy.all(oi[8 + kk:8 + k] == -1)


@pytest.mark.parametrize('status', [0, 1, 2, 4, 5])
def test_a_slot_without_a_region_gets_its_head_only(program, status):
    """what the fetch writes for a candidate the LDS-engine kernel re-solved to another verdict: status, candidate, zero counts, -1 lists"""
    shape = (3, 2, 6, 3, 1, 2)
    rec_d, rec_i = fixed_record(numpy.random.default_rng(1), 3, 2, 6, 3, 2, 4, 1, 1, 2)
    head, od, oi, pool, _, _ = convert(program, shape, rec_d, rec_i, status=status, cand=5, row0=2)
    assert head[7] == 0 and oi[:8].tolist() == [status, 5, 0, 0, 0, 0, 0, 0] and numpy.all(oi[8:] == -1)
    assert numpy.all(od == 7.0) and numpy.all(pool == 9.0)
