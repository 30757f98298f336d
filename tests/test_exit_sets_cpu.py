"""The host side of Solution.exit_sets without a device: the CPU reference on cases worked out by hand (tests/exit_cases.py),
the round driver of exit_sets.exit_pieces over a stand-in for the two device calls built on the reference's LP, ExitSets.contains, and
every refusal that comes before a launch."""
import numpy
import pytest

import exit_cases as ec
import exit_reference as ref
import transition_reference as tref
from ppopt_amd import _lib, exit_sets as ex
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.region_merge import mask_rows
from ppopt_amd.solution import Solution
from ppopt_amd.transition import TransitionGraph

TOL = 1e-8


def _sorted_intervals(pieces):
    return sorted(ec.intervals([(p[0], p[1]) for p in pieces]))


# ---- the reference on the hand cases -------------------------------------------------------------------------------------------------
def test_reference_one_d_mismatched_plant():
    polys, Phi, phi, succ = ec.one_d_loop(4)
    assert ref.successors_reference(polys, Phi, phi, TOL)[0] == succ
    pieces, _ = ref.exit_reference(polys, Phi, phi, succ, TOL)
    got = _sorted_intervals(pieces)
    want = [(0, -0.75, -0.25), (1, -0.25, -0.1875), (1, 0.1875, 0.25), (2, 0.25, 0.75)]
    assert [g[0] for g in got] == [w[0] for w in want]
    numpy.testing.assert_allclose([g[1:] for g in got], [w[1:] for w in want], atol=1e-12)
    assert [p[3] for p in pieces] == [True, False, False, True] and not any(p[2] for p in pieces)
    assert abs(sum(hi - lo for _, lo, hi in got) - 1.125) <= 1e-12
    assert [p[0] for p in pieces] == [0, 1, 1, 2]


def test_reference_one_d_matched_plant_has_no_piece():
    polys, Phi, phi, succ = ec.one_d_loop(2)
    assert ref.successors_reference(polys, Phi, phi, TOL)[0] == succ
    assert ref.exit_reference(polys, Phi, phi, succ, TOL)[0] == []


def test_reference_grid_leaves_through_one_side():
    polys, Phi, phi, succ = ec.grid_shift(0.5)
    assert ref.successors_reference(polys, Phi, phi, TOL)[0] == succ
    pieces, _ = ref.exit_reference(polys, Phi, phi, succ, TOL)
    assert [p[0] for p in pieces] == [2, 5, 8] and not any(p[3] for p in pieces)
    for src, rows, wide, whole in pieces:
        r = src // 3
        open_, rad, centre = tref.chebyshev(rows)
        assert not open_ and abs(rad - 0.25) <= 1e-12 and abs(centre[0] - 2.75) <= 1e-9 and r + 0.25 - 1e-9 <= centre[1] <= r + 0.75 + 1e-9
        corners = numpy.array([[2.5, r], [3, r], [2.5, r + 1], [3, r + 1]])
        assert numpy.all(corners @ rows[:, 1:].T <= rows[:, 0] + 1e-12)


def test_reference_constant_rows_of_each_sign():
    polys, Phi, phi, succ = ec.constant_rows()
    back, empty, knife = tref.pulled_back(polys[1], Phi[0], phi[0], TOL)
    assert len(back) == 2 and not empty and not knife                         # beta = +1/2 twice: dropped
    assert tref.pulled_back(polys[0], Phi[1], phi[1], TOL)[1] and tref.pulled_back(polys[1], Phi[1], phi[1], TOL)[1]      # beta = -1/2
    pieces, _ = ref.exit_reference(polys, Phi, phi, succ, TOL)
    assert [(p[0], p[3]) for p in pieces] == [(1, True)]
    numpy.testing.assert_array_equal(pieces[0][1], polys[1])
    rows = ex.pulled_back_rows(polys[1], Phi[0], phi[0])
    assert numpy.isnan(rows[[1, 3]]).all()
    numpy.testing.assert_allclose(rows[[0, 2]], back, atol=1e-15)


def test_the_first_seed_has_no_knife_region():
    n, seed, k, act, size = ec.SETS[0]
    polys, Phi, phi = ec.synthetic_set(n, seed, k, act, size)
    succ, graph_knife = ref.successors_reference(polys, Phi, phi, TOL)
    pieces, knife = ref.exit_reference(polys, Phi, phi, succ, TOL)
    assert not graph_knife and not knife and len(pieces) > k and not any(p[2] for p in pieces)


# ---- the round driver over a stand-in for the device ------------------------------------------------------------------------------------
def _stand_in(monkeypatch):
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
            if not ref._radius(numpy.vstack([piece, back[keep]]), tol, state)[0]:
                continue
            flag[q] = _lib.OVERLAP_MEETS
            cutting = []
            for k in keep:
                if ref._radius(numpy.vstack([piece] + cutting + [-back[k][None]]), tol, state)[0]:
                    cutting.append(back[k][None])
                    mask[q, k >> 6] |= numpy.uint64(1) << numpy.uint64(k & 63)
        return flag, mask, {'items': n, 'meets': int(numpy.sum(flag != 0)), 'lps': 0, 'pivots': 0, 'wide': 0, 'ms': 0.0}

    monkeypatch.setattr(_lib, 'merge_regions', merge_regions)
    monkeypatch.setattr(_lib, 'exit_split', exit_split)


@pytest.mark.parametrize('case', [lambda: ec.one_d_loop(4), lambda: ec.one_d_loop(2), ec.grid_shift, ec.constant_rows,
                                  lambda: ec.synthetic_set(*ec.SETS[0][:3]) + (None,)], ids=['a4', 'a2', 'grid', 'constant', 'n2'])
def test_driver_gives_the_reference_pieces(monkeypatch, case):
    _stand_in(monkeypatch)
    polys, Phi, phi, succ = case()
    if succ is None:
        succ = ref.successors_reference(polys, Phi, phi, TOL)[0]
    off, ef = ec.csr(polys)
    got = ex.exit_pieces(off, ef, Phi, phi, ef.shape[1] - 1, succ, tol=TOL)
    want, _ = ref.exit_reference(polys, Phi, phi, succ, TOL)
    assert got.source.tolist() == [p[0] for p in want] and len(got) == len(want) and got.n_regions == len(polys)
    for k, (src, rows, wide, whole) in enumerate(want):
        numpy.testing.assert_allclose(got.rows_of(k), rows, rtol=0, atol=1e-12)
    assert got.whole.tolist() == [any(p[0] == i and p[3] for p in want) for i in range(len(polys))]
    assert not got.wide.any() and got.stats['pieces'] == len(want)
    assert got.stats['rounds'] == max(len(s) for s in succ) if any(len(polys[i]) and succ[i] for i in range(len(polys))) else True
    assert [got.pieces_of(i).tolist() for i in range(len(polys))] == [[k for k, p in enumerate(want) if p[0] == i] for i in range(len(polys))]


def test_contains():
    polys, Phi, phi, succ = ec.one_d_loop(4)
    want, _ = ref.exit_reference(polys, Phi, phi, succ, TOL)
    off, rows = ec.csr([p[1] for p in want])
    roff, rrows = ec.csr(polys)
    e = ex.ExitSets(3, off, rows, numpy.array([p[0] for p in want]), numpy.zeros(4, dtype=bool), numpy.array([True, False, True]), {}, roff, rrows)
    th = numpy.array([[-0.5], [-0.2], [0.0], [0.2], [0.5], [0.18], [-0.24], [0.9], [-0.25]])
    got = e.contains(th)
    iv = ec.intervals([(p[0], p[1]) for p in want])
    for t, k in zip(th[:, 0], got):
        inside = [q for q, (_, lo, hi) in enumerate(iv) if lo <= t <= hi]
        assert k == (inside[0] if inside else -1), (t, k)
    assert got[2] == -1 and got[5] == -1 and got[7] == -1 and (got[[0, 1, 3, 4, 6, 8]] >= 0).all()
    assert e.contains([0.19]).tolist() == [got[3]] and e.contains(numpy.zeros((0, 1))).tolist() == []
    assert e.contains([[0.1875 - 1e-7]]).tolist() == [-1] and e.contains([[0.1875 - 1e-7]], tol=1e-6).tolist() == [got[3]]
    with pytest.raises(ValueError, match='thetas must be'):
        e.contains(numpy.zeros((2, 2)))
    assert len(e.polytopes()) == 4 and e.polytopes()[1].A.shape[1] == 1
    empty = ex.ExitSets(3, numpy.zeros(1, dtype=numpy.int64), numpy.zeros((0, 2)), numpy.zeros(0, dtype=numpy.int64), numpy.zeros(0, dtype=bool),
                        numpy.zeros(3, dtype=bool), {}, roff, rrows)
    assert empty.contains(th).tolist() == [-1] * len(th) and len(empty) == 0


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------------
class _Prog:
    def __init__(self, n_t):
        self._nt = n_t

    def num_t(self):
        return self._nt


def _stub(n_t=2, n_regions=2, overlapping=False, mixed=False, rows=4):
    regs = []
    for i in range(n_regions):
        E = numpy.vstack([numpy.eye(n_t), -numpy.eye(n_t)] * (rows // 4 + 1))[:max(rows, 2 * n_t)]
        r = CriticalRegion(numpy.zeros((3, n_t)), numpy.zeros((3, 1)), numpy.zeros((0, n_t)), numpy.zeros((0, 1)), E, numpy.ones((len(E), 1)), [i])
        if mixed:
            r.y_fixation, r.y_indices, r.x_indices = numpy.array([1.0]), [3], [0, 1, 2]
        regs.append(r)
    return Solution(_Prog(n_t), regs, is_overlapping=overlapping)


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the device was touched')
    for name in ('merge_regions', 'transition_boxes', 'transition_pairs', 'exit_split', 'load'):
        monkeypatch.setattr(_lib, name, boom)


def test_exit_sets_refusals(monkeypatch):
    _no_device(monkeypatch)
    A, B = numpy.eye(2), numpy.ones((2, 1))
    good = _stub()
    for sol, args, kw, text in ((_stub(mixed=True), (A, B, [0]), {}, 'mixed-integer'),
                                (_stub(overlapping=True), (A, B, [0]), {}, 'remove_overlaps'),
                                (Solution(_Prog(2), []), (A, B, [0]), {}, 'no region'),
                                (good, (numpy.eye(3), B, [0]), {}, r'A must be \[2, 2\]'),
                                (good, (A, numpy.ones((3, 1)), [0]), {}, 'B must be'),
                                (good, (A, B, [3]), {}, 'out of range'),
                                (good, (A, B, [0, 1]), {}, 'inputs must be 1 integer'),
                                (good, (A * numpy.nan, B, [0]), {}, 'A must be finite'),
                                (good, (A, B, [0]), {'c': [0.0]}, 'c must have 2 entries'),
                                (good, (A, B, [0]), {'tol': -1.0}, 'tol must be finite'),
                                (good, (A, B, [0]), {'tol': numpy.nan}, 'tol must be finite'),
                                (_stub(rows=260), (A, B, [0]), {}, 'more than 256 rows'),
                                (_stub(n_t=17), (numpy.eye(17), numpy.ones((17, 1)), [0]), {}, 'n_theta = 17 > 16'),
                                (good, (A, B, [0]), {'max_pieces': 0}, 'max_pieces must be >= 1'),
                                (good, (A, B, [0]), {'graph': TransitionGraph.from_edges(3, [0], [1])}, 'the graph has 3 regions, the solution 2')):
        with pytest.raises(ValueError, match=text):
            sol.exit_sets(*args, **kw)


def test_exit_pieces_refuses_bad_arrays_on_the_host(monkeypatch):
    _no_device(monkeypatch)
    sq = ec.box_rows([0, 0], [1, 1])
    off, ef = numpy.array([0, 4, 8]), numpy.vstack([sq, sq])
    Phi, phi = numpy.tile(numpy.eye(2), (2, 1, 1)), numpy.zeros((2, 2))
    for kw, text in (({'tol': -1.0}, 'tol'), ({'tol': numpy.inf}, 'tol'), ({'Phi': Phi[:1]}, 'must describe'), ({'phi': phi * numpy.nan}, 'finite'),
                     ({'Phi': Phi * numpy.inf}, 'finite'), ({'ef': ef * numpy.nan}, 'finite'), ({'n_t': 0}, 'outside 1..16'),
                     ({'off': numpy.array([0, 0, 8])}, '1..256 rows'), ({'off': numpy.array([1, 4, 8])}, 'must describe'),
                     ({'succ': [[0]]}, 'one index list per polytope'), ({'succ': [[0], [2]]}, 'must name polytopes 0..1'),
                     ({'succ': [[-1], []]}, 'must name polytopes 0..1'), ({'max_pieces': 0}, 'max_pieces')):
        a = dict(off=off, ef=ef, Phi=Phi, phi=phi, n_t=2, tol=TOL, succ=[[0], [1]], max_pieces=4)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ex.exit_pieces(a['off'], a['ef'], a['Phi'], a['phi'], a['n_t'], a['succ'], tol=a['tol'], max_pieces=a['max_pieces'])
    with pytest.raises(ValueError, match='outside 1..16'):
        ex.exit_pieces(numpy.array([0, 4]), numpy.hstack([numpy.ones((4, 1)), numpy.eye(17)[:4]]), numpy.eye(17)[None], numpy.zeros((1, 17)), 17, [[]])


def test_the_piece_limits_raise_after_the_round(monkeypatch):
    _stand_in(monkeypatch)
    polys, Phi, phi, succ = ec.one_d_loop(4)
    off, ef = ec.csr(polys)
    with pytest.raises(ValueError, match='more than max_pieces = 3 pieces after round 1'):
        ex.exit_pieces(off, ef, Phi, phi, 1, succ, tol=TOL, max_pieces=3)
    # a region of 256 rows whose cutter cuts: the child would have 257
    n = 128
    ang = numpy.arange(2 * n) * numpy.pi / n
    disc = numpy.column_stack([numpy.ones(2 * n), numpy.cos(ang), numpy.sin(ang)])
    off, ef = ec.csr([disc, ec.box_rows([0.5, -2], [3, 2])])
    with pytest.raises(ValueError, match='a piece has more than 256 rows after round 1'):
        ex.exit_pieces(off, ef, numpy.tile(numpy.eye(2), (2, 1, 1)), numpy.zeros((2, 2)), 2, [[1], []], tol=TOL)


def test_the_abi_names():
    assert 'mpc_exit_split' in _lib.EXPORTED_SYMBOLS and (_lib.OVERLAP_MEETS, _lib.OVERLAP_WIDE) == (1, 4)
    assert mask_rows(numpy.array([5, 0, 0, 1], dtype=numpy.uint64), 256).tolist() == [0, 2, 192]
