"""Removing redundant rows without a device: the CPU reference on cases whose masks are derived by hand
(tests/reduce_cases.py), the host layer and the round driver over a stand-in for _lib.reduce_rows built on the reference, and every
refusal that comes before a launch."""
import numpy
import pytest

import exit_cases as ec
import exit_reference as eref
import reduce_cases as rc
import reduce_reference as rr
import transition_reference as tref
from ppopt_amd import _lib, exit_sets as ex, overlap
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.geometry import Polytope, ReducedRows, reduce_polytopes, reduce_rows_of
from ppopt_amd.region_merge import build_merged_solution
from ppopt_amd.solution import Solution

TOL = rc.TOL
BAND = 1e-6


# ---- the reference on the hand cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,rows,kept,thin', rc.hand_cases(), ids=[c[0] for c in rc.hand_cases()])
def test_reference_on_the_hand_cases(name, rows, kept, thin):
    r = rr.reduce_one(rows, TOL)
    assert r.kept.tolist() == [bool(k) for k in kept] and r.thin == thin and not r.knife
    assert r.wide == (1 if name == 'interval' else 0)
    if thin:
        assert numpy.all(numpy.isnan(r.row_radius)) and abs(r.radius) <= 1e-9
    if name == 'touching':
        assert abs(r.row_radius[4]) <= 1e-9
    if name == 'twice':
        assert abs(r.row_radius[0]) <= 1e-9 and abs(r.row_radius[4] - 0.5) <= 1e-9
    if name == 'outside':
        assert r.row_radius[4] < -0.4


@pytest.mark.parametrize('case', rc.SETS[:3], ids=rc.IDS[:3])
def test_the_small_seeds_have_no_knife_polytope_and_no_unbounded_run(case):
    polys = rc.seeded_set(*case)
    res = rr.reduce_reference(polys, TOL)
    assert len(polys) == case[2] and all(case[3][0] <= len(p) <= case[3][1] for p in polys)
    assert not any(r.knife for r in res) and not any(r.wide for r in res) and not any(r.thin for r in res)
    removed = sum(int((~r.kept).sum()) for r in res)
    assert removed >= 2 * len(polys)           # at least the outside row and the copy of every polytope


# ---- the host layer over a stand-in for the device ---------------------------------------------------------------------------------------
def _reduce_stand_in(monkeypatch, calls=None):
    """_lib.reduce_rows answered by the reference, in the terms of the binding: (kept per row, status, wide, point, stats)"""
    def reduce_rows(off, ef, start, tol, device=0):
        off, ef = numpy.asarray(off), numpy.asarray(ef)
        n = len(off) - 1
        res = [rr.reduce_one(ef[off[q]:off[q + 1]], tol) for q in range(n)]
        if calls is not None:
            calls.append((n, None if start is None else numpy.array(start, copy=True), [r.wide for r in res]))
        point = numpy.zeros((n, ef.shape[1] - 1)) if start is None else numpy.array(start, dtype=float, copy=True)
        lps = sum(1 + int(numpy.sum(~numpy.isnan(r.row_radius))) for r in res)
        return (numpy.concatenate([r.kept for r in res]) if n else numpy.zeros(0, dtype=bool),
                numpy.array([_lib.REDUCE_THIN if r.thin else _lib.REDUCE_OK for r in res], dtype=numpy.int32),
                numpy.array([r.wide for r in res], dtype=numpy.int32), point,
                {'polytopes': n, 'thin': sum(r.thin for r in res), 'lps': lps, 'pivots': 0, 'wide': sum(r.wide for r in res), 'ms': 0.0})
    monkeypatch.setattr(_lib, 'reduce_rows', reduce_rows)


def _difference_stand_in(monkeypatch):
    """_lib.merge_regions and _lib.exit_split answered by the reference's LP, in the ABI's terms (flag bits, row mask)"""
    def merge_regions(off, ef, device=0):
        R = len(off) - 1
        xs, st = numpy.zeros((R, ef.shape[1] - 1)), numpy.zeros(R, dtype=numpy.int32)
        for i in range(R):
            open_, r, th = tref.chebyshev(ef[off[i]:off[i + 1]])
            st[i] = 0 if open_ or r >= 0 else 1
            if th is not None:
                xs[i] = th
        return xs, None, st, {'lps': 0, 'pivots': 0, 'capped': 0, 'ms': 0.0}

    def exit_split(off, ef, Phi, phi, poff, prow, item_piece, item_source, item_target, start, tol, device=0):
        n = len(item_piece)
        flag, mask = numpy.zeros(n, dtype=numpy.int32), numpy.zeros((n, _lib.MERGE_WORDS), dtype=numpy.uint64)
        for q, (p, i, j) in enumerate(zip(item_piece, item_source, item_target)):
            piece, target = prow[poff[p]:poff[p + 1]], ef[off[j]:off[j + 1]]
            back = ex.pulled_back_rows(target, Phi[i], phi[i])
            if tref.pulled_back(target, Phi[i], phi[i], tol)[1]:
                continue
            keep = numpy.flatnonzero(~numpy.isnan(back[:, 0]))
            state = {'knife': False}
            if not eref._radius(numpy.vstack([piece, back[keep]]), tol, state)[0]:
                continue
            flag[q] = _lib.OVERLAP_MEETS
            cutting = []
            for k in keep:
                if eref._radius(numpy.vstack([piece] + cutting + [-back[k][None]]), tol, state)[0]:
                    cutting.append(back[k][None])
                    mask[q, k >> 6] |= numpy.uint64(1) << numpy.uint64(k & 63)
        return flag, mask, {'items': n, 'meets': int(numpy.sum(flag != 0)), 'lps': 0, 'pivots': 0, 'wide': 0, 'ms': 0.0}

    monkeypatch.setattr(_lib, 'merge_regions', merge_regions)
    monkeypatch.setattr(_lib, 'exit_split', exit_split)


def test_reduce_rows_of_keeps_order_bits_and_the_source(monkeypatch):
    _reduce_stand_in(monkeypatch)
    cases = [c for c in rc.hand_cases() if c[1].shape[1] == 3]
    off, ef = ec.csr([c[1] for c in cases])
    before = (off.copy(), ef.copy())
    r = reduce_rows_of(off, ef, 2, tol=TOL)
    assert isinstance(r, ReducedRows) and len(r) == len(cases)
    assert off.tobytes() == before[0].tobytes() and ef.tobytes() == before[1].tobytes()
    want = numpy.concatenate([numpy.asarray(c[2], dtype=bool) for c in cases])
    assert r.kept.dtype == bool and r.kept.tolist() == want.tolist()
    assert r.rows.tobytes() == ef[want].tobytes()                                   # order and bits
    assert r.row_off.tolist() == numpy.concatenate([[0], numpy.cumsum([sum(c[2]) for c in cases])]).tolist()
    assert r.status.tolist() == [_lib.REDUCE_THIN if c[3] else _lib.REDUCE_OK for c in cases] and not r.wide.any()
    assert r.point.shape == (len(cases), 2)
    s = r.stats
    assert s['rows_before'] == len(ef) and s['rows_after'] == int(want.sum()) and s['thin'] == 1 and s['polytopes'] == len(cases)
    assert s['lps'] == sum(1 + (0 if c[3] else len(c[1])) for c in cases) and {'pivots', 'device_ms', 'wall_ms'} <= set(s)
    numpy.testing.assert_array_equal(r.rows_of(3), cases[3][1][1:])
    assert [p.A.shape for p in r.polytopes()] == [(int(sum(c[2])), 2) for c in cases]


def test_polytopes_are_scaled_first_and_keep_their_own_rows(monkeypatch):
    _reduce_stand_in(monkeypatch)
    sq = ec.box_rows([0, 0], [1, 1])
    A = numpy.vstack([sq[:, 1:], [[3.0, 0.0]]]) * numpy.array([[2.0], [1.0], [0.5], [7.0], [1.0]])
    b = numpy.concatenate([sq[:, 0], [6.0]]).reshape(-1, 1) * numpy.array([[2.0], [1.0], [0.5], [7.0], [1.0]])
    p = Polytope(A.copy(), b.copy())
    q = p.reduced(tol=TOL)
    assert q.A.tobytes() == A[:4].tobytes() and q.b.tobytes() == b[:4].tobytes() and p.A.tobytes() == A.tobytes()
    r = reduce_polytopes([p, Polytope(sq[:, 1:], sq[:, :1])], tol=TOL)
    assert r.kept.tolist() == [True] * 4 + [False] + [True] * 4
    numpy.testing.assert_allclose(numpy.linalg.norm(r.rows[:, 1:], axis=1), 1.0, rtol=0, atol=1e-15)


def test_exit_sets_reduced_keeps_everything_but_the_rows(monkeypatch):
    _reduce_stand_in(monkeypatch)
    sq = ec.box_rows([0, 0], [1, 1])
    pieces = [numpy.vstack([sq, rc.hand_cases()[0][1][4]]), rc.hand_cases()[3][1], sq]
    off, rows = ec.csr(pieces)
    roff, rrows = ec.csr([sq, sq + numpy.array([1.0, 0, 0])])
    e = ex.ExitSets(2, off, rows, numpy.array([0, 0, 1]), numpy.array([False, True, False]), numpy.array([False, True]), {'lps': 7, 'rounds': 1}, roff, rrows,
                    tol=TOL)
    before = (off.copy(), rows.copy())
    got = e.reduced()
    assert off.tobytes() == before[0].tobytes() and rows.tobytes() == before[1].tobytes() and e.stats == {'lps': 7, 'rounds': 1}
    assert got.piece_off.tolist() == [0, 4, 8, 12] and got.piece_rows.tobytes() == numpy.vstack([sq, rc.hand_cases()[3][1][1:], sq]).tobytes()
    assert got.source.tolist() == [0, 0, 1] and got.wide.tolist() == [False, True, False] and got.whole.tolist() == [False, True]
    assert got.region_off is roff and got.region_rows is rrows and got.n_regions == 2 and got.tol == TOL
    assert got.stats['lps'] == 7 and got.stats['rows_removed'] == 2 and got.stats['reduce_lps'] == 3 + 5 + 5 + 4 and 'reduce_ms' in got.stats
    assert got.reduced(tol=TOL).stats['rows_removed'] == 0
    empty = ex.ExitSets(2, numpy.zeros(1, dtype=numpy.int64), numpy.zeros((0, 3)), numpy.zeros(0, dtype=numpy.int64), numpy.zeros(0, dtype=bool),
                        numpy.zeros(2, dtype=bool), {}, roff, rrows)
    assert len(empty.reduced()) == 0 and empty.reduced().stats['rows_removed'] == 0


class _Prog:
    def __init__(self, n_t):
        self._nt = n_t

    def num_t(self):
        return self._nt


def _source(n_regions=2, n_t=2):
    regs = []
    for i in range(n_regions):
        sq = ec.box_rows(numpy.full(n_t, float(i)), numpy.full(n_t, i + 1.0))
        regs.append(CriticalRegion(numpy.full((3, n_t), i + 1.0), numpy.full((3, 1), float(i)), numpy.ones((1, n_t)), numpy.ones((1, 1)), sq[:, 1:], sq[:, :1], [i]))
    sol = Solution(_Prog(n_t), regs)
    sol.is_complete = True
    return sol


def test_solution_reduce_rows_replaces_only_E_and_f(monkeypatch):
    _reduce_stand_in(monkeypatch)
    src = _source()
    sq0, sq1 = ec.box_rows([0, 0], [1, 1]), ec.box_rows([1, 1], [2, 2])
    # piece 0: the square with x <= 2 and a copy of its first row; piece 1: source 1 untouched (None); the rows of piece 0 are not unit
    scale = numpy.array([[3.0], [1.0], [0.25], [1.0], [2.0], [5.0]])
    p0 = numpy.vstack([sq0, [[2.0, 1.0, 0.0]], sq0[:1]])
    red = overlap.build_reduced_solution(src, [0, 1], [p0, None], {'CROSSING': 1}, [], {'lps': 3})
    red.critical_regions[0].E, red.critical_regions[0].f = p0[:, 1:] * scale, p0[:, :1] * scale
    E0, f0 = red.critical_regions[0].E.copy(), red.critical_regions[0].f.copy()
    out = red.reduce_rows(tol=TOL)
    assert out is not red and len(out) == 2 and out.overlap_info is red.overlap_info and out.merge_info is None
    assert out.is_complete and out.is_overlapping == red.is_overlapping and out.point_location_tolerance == red.point_location_tolerance
    keep = [1, 2, 3, 5]                                     # row 0 falls to its copy, row 4 (x <= 2) is outside
    a, b = out.critical_regions[0], red.critical_regions[0]
    assert a.E.tobytes() == E0[keep].tobytes() and a.f.tobytes() == f0[keep].tobytes()
    assert b.E.tobytes() == E0.tobytes() and b.f.tobytes() == f0.tobytes() and a is not b                  # the source keeps its rows
    for name in ('A', 'b', 'C', 'd'):
        numpy.testing.assert_array_equal(getattr(a, name), getattr(b, name))
    assert a.active_set == b.active_set and a.source == b.source == 0 and type(a) is type(b)
    numpy.testing.assert_array_equal(out.critical_regions[1].E, sq1[:, 1:])
    info = out.reduce_info
    assert info['source'] is red and info['kept'].tolist() == [False, True, True, True, False, True] + [True] * 4 and info['stats']['rows_after'] == 8
    merged = build_merged_solution(src, [[0], [1]], [p0, None], [0])
    again = merged.reduce_rows(tol=TOL)
    assert again.merge_info is merged.merge_info and again.critical_regions[0].members == [0]
    assert again.critical_regions[0].E.tobytes() == p0[keep, 1:].tobytes() and len(merged.critical_regions[0].E) == 6


# ---- the round driver ---------------------------------------------------------------------------------------------------------------------
def _chebyshev_pieces(pieces):
    out = []
    for rows in pieces:
        _, r, centre = tref.chebyshev(rows)
        out.append((rows, r, centre))
    return out


def same_sets(mine, theirs, band=BAND):
    """the two-sided centre test of tests/test_gpu_exit_sets.py: each side's pieces of radius above the band have their Chebyshev centre
    in a piece of the other side"""
    a, b = _chebyshev_pieces(mine), _chebyshev_pieces(theirs)
    for one, other in ((a, b), (b, a)):
        for rows, r, centre in one:
            if r > band:
                assert any(numpy.all(q[:, 1:] @ centre <= q[:, 0] + 1e-9) for q, _, _ in other), r
    return sum(r > band for _, r, _ in a), sum(r > band for _, r, _ in b)


def test_the_row_limit_falls_with_reduce_and_stands_without(monkeypatch):
    """a source of 250 rows and a cutter of 8: the children have up to 258 rows, and each is a polygon of far fewer sides"""
    _difference_stand_in(monkeypatch)
    calls = []
    _reduce_stand_in(monkeypatch, calls)
    polys, Phi, phi, succ = rc.many_rows_difference(250, 8)
    off, ef = ec.csr(polys)
    with pytest.raises(ValueError, match='exit_sets: a piece has more than 256 rows after round 1'):
        ex.exit_pieces(off, ef, Phi, phi, 2, succ, tol=TOL)
    assert not calls
    got = ex.exit_pieces(off, ef, Phi, phi, 2, succ, tol=TOL, reduce_rows=True)
    want, knife = eref.exit_reference(polys, Phi, phi, succ, TOL)          # the difference without a row limit
    assert not knife and max(len(p[1]) for p in want) == 258
    assert got.source.tolist() == [p[0] for p in want] == [0] * 8 + [1] and got.whole.tolist() == [False, True]
    # (a run beyond the last row of the source's arc that a child keeps is unbounded: the row is kept and the piece flagged, the safe way)
    assert got.wide.tolist() == [w > 0 for w in calls[0][2]] + [False]
    assert int(numpy.diff(got.piece_off).max()) <= 256 and len(got.rows_of(8)) == 8
    n_mine, n_theirs = same_sets([got.rows_of(k) for k in range(len(got))], [p[1] for p in want])
    assert n_mine == n_theirs == 9
    # one call per round over the new children only, started from the source's point
    assert len(calls) == 1 and calls[0][0] == 8 and numpy.all(calls[0][1] == calls[0][1][0]) and numpy.all(numpy.abs(calls[0][1]) < 1.0)
    s = got.stats
    assert s['rows_removed'] == sum(len(p[1]) for p in want[:8]) - int(got.piece_off[8]) > 8 * 100 and s['reduce_lps'] > 8 * 250 and s['reduce_ms'] == 0.0
    # every kept row is one of the child's rows, bit for bit and in order
    for k in range(8):
        child, mine = want[k][1], got.rows_of(k)
        at = [int(numpy.flatnonzero(numpy.all(child == row, axis=1))[0]) for row in mine]
        assert at == sorted(at)


def test_a_thin_child_is_dropped_and_a_wide_one_flags_its_piece(monkeypatch):
    _difference_stand_in(monkeypatch)
    polys, Phi, phi, succ = ec.grid_shift(0.5)
    off, ef = ec.csr(polys)
    plain = ex.exit_pieces(off, ef, Phi, phi, 2, succ, tol=1e-8)
    assert plain.source.tolist() == [2, 5, 8]

    calls = []

    def reduce_rows(off_, ef_, start, tol, device=0):
        # round 1 makes one child per cell, [c + 1/2, c + 1] x [r, r + 1]: the child of cell 2 is called thin, the one of cell 5 loses its
        # first row, the one of cell 8 had two unbounded runs; the children of the columns 0 and 1 vanish in round 2, which makes none
        n = len(off_) - 1
        calls.append(n)
        kept, status, wide = numpy.ones(len(ef_), dtype=bool), numpy.zeros(n, dtype=numpy.int32), numpy.zeros(n, dtype=numpy.int32)
        kept[off_[5]], status[2], wide[8] = False, _lib.REDUCE_THIN, 2
        return kept, status, wide, numpy.zeros((n, 2)), {'polytopes': n, 'thin': 1, 'lps': 5, 'pivots': 0, 'wide': 2, 'ms': 0.25}
    monkeypatch.setattr(_lib, 'reduce_rows', reduce_rows)
    got = ex.exit_pieces(off, ef, Phi, phi, 2, succ, tol=1e-8, reduce_rows=True)
    assert got.source.tolist() == [5, 8] and got.wide.tolist() == [False, True]
    assert got.rows_of(0).tobytes() == plain.rows_of(1)[1:].tobytes() and got.rows_of(1).tobytes() == plain.rows_of(2).tobytes()
    assert calls == [9] and got.stats['rows_removed'] == 1 and got.stats['reduce_lps'] == 5 and got.stats['reduce_ms'] == 0.25


@pytest.mark.parametrize('case', [lambda: ec.one_d_loop(4), ec.grid_shift, lambda: ec.synthetic_set(*ec.SETS[0][:3]) + (None,)], ids=['a4', 'grid', 'n2'])
def test_without_reduce_the_driver_is_what_it_was(monkeypatch, case):
    _difference_stand_in(monkeypatch)
    monkeypatch.setattr(_lib, 'reduce_rows', lambda *a, **k: pytest.fail('reduce_rows was called'))
    polys, Phi, phi, succ = case()
    if succ is None:
        succ = eref.successors_reference(polys, Phi, phi, 1e-8)[0]
    off, ef = ec.csr(polys)
    got = ex.exit_pieces(off, ef, Phi, phi, ef.shape[1] - 1, succ, tol=1e-8)
    same = ex.exit_pieces(off, ef, Phi, phi, ef.shape[1] - 1, succ, tol=1e-8, reduce_rows=False)
    want, _ = eref.exit_reference(polys, Phi, phi, succ, 1e-8)
    assert got.source.tolist() == [p[0] for p in want]
    for k, (src, rows, wide, whole) in enumerate(want):
        numpy.testing.assert_allclose(got.rows_of(k), rows, rtol=0, atol=1e-12)
    for name in ('piece_off', 'piece_rows', 'source', 'wide', 'whole'):
        assert getattr(got, name).tobytes() == getattr(same, name).tobytes()
    assert set(got.stats) == {'rounds', 'items', 'lps', 'pivots', 'wide', 'device_ms', 'round_ms', 'max_item_rows', 'pieces', 'wall_ms'}


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the device was touched')
    for name in ('reduce_rows', 'merge_regions', 'exit_split', 'overlap_split', 'load'):
        monkeypatch.setattr(_lib, name, boom)


def test_refusals_on_the_host(monkeypatch):
    _no_device(monkeypatch)
    sq = ec.box_rows([0, 0], [1, 1])
    off, ef = numpy.array([0, 4, 8]), numpy.vstack([sq, sq])
    big = numpy.tile(sq, (129, 1))
    for kw, text in (({'n_t': 0}, 'outside 1..16'), ({'n_t': 17}, 'outside 1..16'), ({'tol': -1.0}, 'tol must be finite'), ({'tol': numpy.nan}, 'tol must be finite'),
                     ({'tol': numpy.inf}, 'tol must be finite'), ({'off': numpy.array([0, 0, 8])}, '1..512 rows'), ({'off': numpy.array([0, 516]), 'ef': big}, '1..512 rows'),
                     ({'off': numpy.array([1, 4, 8])}, 'row_off'), ({'off': numpy.array([0, 4, 7])}, 'row_off'), ({'off': numpy.array([0])}, 'row_off'),
                     ({'ef': ef * numpy.nan}, 'finite'), ({'ef': ef * 2.0}, 'unit normals'), ({'ef': ef[:, :2]}, r'ef_rows must be \[rows, 3\]'),
                     ({'start': numpy.zeros((3, 2))}, 'start must be'), ({'start': numpy.full((2, 2), numpy.inf)}, 'start must be')):
        a = dict(off=off, ef=ef, n_t=2, tol=TOL, start=None)
        a.update(kw)
        with pytest.raises(ValueError, match='reduce_rows_of: .*' + text):
            reduce_rows_of(a['off'], a['ef'], a['n_t'], tol=a['tol'], start=a['start'])
    with pytest.raises(ValueError, match='reduce_polytopes: no polytopes'):
        reduce_polytopes([])
    with pytest.raises(ValueError, match='different dimensions'):
        reduce_polytopes([Polytope(sq[:, 1:], sq[:, :1]), Polytope(numpy.array([[1.0], [-1.0]]), numpy.ones((2, 1)))])
    with pytest.raises(ValueError, match='Polytope.reduced: .*zero row'):
        Polytope(numpy.vstack([sq[:, 1:], [[0.0, 0.0]]]), numpy.ones((5, 1))).reduced()
    with pytest.raises(ValueError, match='A has shape'):
        Polytope(sq[:, 1:], numpy.ones((3, 1))).reduced()
    with pytest.raises(ValueError, match='Polytope.reduced: tol must be finite'):
        Polytope(sq[:, 1:], sq[:, :1]).reduced(tol=-1.0)
    roff, rrows = ec.csr([sq])
    e = ex.ExitSets(1, numpy.array([0, 4]), sq, numpy.array([0]), numpy.zeros(1, dtype=bool), numpy.ones(1, dtype=bool), {}, roff, rrows)
    with pytest.raises(ValueError, match='ExitSets.reduced: tol must be finite'):
        e.reduced(tol=numpy.nan)
    src = _source()
    with pytest.raises(ValueError, match='reduce_rows: only the results of merge_regions and remove_overlaps'):
        src.reduce_rows()
    with pytest.raises(ValueError, match='reduce_rows: the solution has no regions'):
        Solution(_Prog(2), []).reduce_rows()
    red = overlap.build_reduced_solution(src, [0, 1], [None, None])
    with pytest.raises(ValueError, match='reduce_rows: tol must be finite'):
        red.reduce_rows(tol=-1e-3)
    red.critical_regions[1].E, red.critical_regions[1].f = big[:516, 1:], big[:516, :1]
    with pytest.raises(ValueError, match='reduce_rows: region 1 has more than 512 rows'):
        red.reduce_rows()
    red.critical_regions[1].E, red.critical_regions[1].f = numpy.zeros((2, 2)), numpy.ones((2, 1))
    with pytest.raises(ValueError, match='reduce_rows: region 1 has no row with a normal'):
        red.reduce_rows()
    wide = overlap.build_reduced_solution(_source(n_t=17), [0, 1], [None, None])
    with pytest.raises(ValueError, match='reduce_rows: n_theta = 17 > 16'):
        wide.reduce_rows()


def test_the_abi_names():
    assert 'mpc_reduce_rows' in _lib.EXPORTED_SYMBOLS
    assert (_lib.REDUCE_MAX_ROWS, _lib.REDUCE_WORDS, _lib.REDUCE_OK, _lib.REDUCE_THIN) == (512, 8, 0, 1)
