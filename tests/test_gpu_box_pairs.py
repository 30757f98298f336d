"""The candidate sweep and the row screen on the device (csrc/box_pairs.hpp, ppopt_amd/geometry/box_pairs.py) against the
numpy references of box_pairs_reference.py, and the sweep= / screen= arguments of compare, transition_graph and remove_overlaps against
their host-sweep results."""
import functools
import warnings

import numpy
import pytest

import box_pairs_reference as ref
import compare_cases as cases
from ppopt_amd import MPQP_Program, Solution, _lib, compare as cmp, overlap, problem_generator as pg, transition as tr
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.geometry import box_pairs, screen_pairs
from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp

pytestmark = pytest.mark.gpu

TOL = ref.TOL
LP_TOL = 1e-8
INF, NAN = numpy.inf, numpy.nan
# below, at and across a wavefront (64), a workgroup (256 rows), a b-tile and a segment boundary (128 boxes); (3, 8300): 65 tiles in 33
# segments of two tiles, the only size here at which a segment holds more than one tile
SIZES = [(1, 1), (65, 63), (257, 130)]


def _same(got, want):
    for g, w in zip(got[:2], want):
        assert g.dtype == numpy.int64 and g.shape == w.shape and numpy.array_equal(g, w)


@functools.lru_cache(maxsize=None)
def _boxes(R, n_t, seed):
    return ref.dyadic_boxes(R, n_t, seed)


# ---- 1. the dyadic boxes: values, dtype and order, exactly ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n_t', [1, 2, 5, 16])
@pytest.mark.parametrize('ra,rb', SIZES)
def test_dyadic_boxes_equal_the_reference(n_t, ra, rb):
    a, b = _boxes(ra, n_t, 10 * n_t + 1), _boxes(rb, n_t, 10 * n_t + 2)
    ua, ub = numpy.arange(ra) % 7 != 3, numpy.arange(rb) % 5 != 1
    for margin in (TOL, -TOL):
        got = box_pairs(a, ua, b, ub, margin=margin)
        want = ref.all_pairs(a, ua, b, ub, margin)
        _same(got, want)
        assert got[2]['pairs'] == len(want[0]) and got[2]['tests'] == int(ua.sum()) * int(ub.sum())
        up = box_pairs(a, ua, margin=margin)
        _same(up, ref.all_pairs(a, ua, margin=margin))
        assert up[2]['tests'] == int(ua.sum()) * (int(ua.sum()) - 1) // 2
    both = box_pairs(a, ua, a, ua, margin=TOL)                     # CROSS with a = b lists i = j (of the boxes that are wider than tol)
    _same(both, ref.all_pairs(a, ua, a, ua, TOL))
    if ra > 1:
        assert numpy.any(both[0] == both[1]) and numpy.any(both[0] > both[1])


def test_segments_of_several_tiles():
    a, b = _boxes(3, 2, 5), _boxes(8300, 2, 6)
    ua, ub = numpy.ones(3, dtype=bool), numpy.arange(8300) % 3 != 0
    got = box_pairs(a, ua, b, ub, margin=-TOL)
    _same(got, ref.all_pairs(a, ua, b, ub, -TOL))
    assert got[2]['segments'] == 33 and got[2]['pairs'] > 1000
    _same(box_pairs(b, ub, a, ua, margin=TOL), ref.all_pairs(b, ub, a, ua, TOL))      # 33 row blocks against one tile
    _same(box_pairs(b[:600], ub[:600], margin=TOL), ref.all_pairs(b[:600], ub[:600], margin=TOL))      # UPPER skips the tiles below the diagonal


# ---- 2. inputs that stress the write offsets -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_t', [2, 16])
def test_write_offsets(n_t):
    ra, rb = 257, 130
    one = numpy.stack([numpy.zeros(n_t), numpy.ones(n_t)])
    a, b = numpy.tile(one, (ra, 1, 1)), numpy.tile(one, (rb, 1, 1))
    all_a, all_b = numpy.ones(ra, dtype=bool), numpy.ones(rb, dtype=bool)
    pa, pb, st = box_pairs(a, all_a, b, all_b, margin=TOL)                     # all boxes equal: every offset of the scan is used
    assert st['pairs'] == len(pa) == ra * rb == 33410
    assert numpy.array_equal(pa, numpy.repeat(numpy.arange(ra), rb)) and numpy.array_equal(pb, numpy.tile(numpy.arange(rb), ra))
    pa, pb, st = box_pairs(a, all_a, margin=TOL)
    iu = numpy.triu_indices(ra, k=1)
    assert numpy.array_equal(pa, iu[0]) and numpy.array_equal(pb, iu[1]) and st['tests'] == st['pairs'] == ra * (ra - 1) // 2
    apart = a + 2.0 * numpy.arange(ra)[:, None, None]                          # all boxes disjoint
    pa, pb, st = box_pairs(apart, all_a, margin=-TOL)
    assert len(pa) == len(pb) == 0 and pa.dtype == numpy.int64 and st['pairs'] == 0 and st['tests'] == ra * (ra - 1) // 2
    even_a, even_b = numpy.arange(ra) % 2 == 0, numpy.arange(rb) % 2 == 0      # every second box unusable
    got = box_pairs(a, even_a, b, even_b, margin=TOL)
    _same(got, ref.all_pairs(a, even_a, b, even_b, TOL))
    assert got[2]['pairs'] == int(even_a.sum()) * int(even_b.sum())
    for ua, ub in ((~all_a, all_b), (all_a, ~all_b)):                          # a family with no usable box: no pair, no launch
        pa, pb, st = box_pairs(a, ua, b, ub, margin=TOL)
        assert len(pa) == len(pb) == 0 and st['tests'] == 0 and st['pairs'] == 0 and st['segments'] == 0 and st['ms'] == 0.0
    counts, st = box_pairs(a, ~all_a, count_only=True)
    assert numpy.array_equal(counts, numpy.zeros(ra, dtype=numpy.int64)) and st['tests'] == 0


# ---- 3. special bounds ---------------------------------------------------------------------------------------------------------------------
def test_nan_and_infinite_bounds():
    whole = [[-INF, -INF], [INF, INF]]
    fam = numpy.array([[[0.0, 0.0], [1.0, 1.0]], whole, [[2.0, -INF], [INF, 0.5]], [[0.5, 0.5], [NAN, 0.75]], [[NAN, 3.0], [0.25, 4.0]],
                       [[0.5, INF], [0.75, INF]], [[0.5, 0.25], [NAN, 0.75]], [[NAN, NAN], [NAN, NAN]], [[INF, 0.0], [-INF, 1.0]]])
    use = numpy.ones(len(fam), dtype=bool)
    for margin in (TOL, -TOL):
        _same(box_pairs(fam, use, fam, use, margin=margin), ref.all_pairs(fam, use, fam, use, margin))
        _same(box_pairs(fam, use, margin=margin), ref.all_pairs(fam, use, margin=margin))
    got = box_pairs(fam, use, fam, use, margin=TOL)
    pairs = set(zip(got[0].tolist(), got[1].tolist()))
    assert (1, 1) in pairs and (7, 7) in pairs and (1, 7) in pairs            # the whole space, and the all-NaN box that reads as it
    assert (1, 5) not in pairs and (5, 5) not in pairs                        # inf - inf fails
    # the whole-space box against everything: every usable box, whatever its size
    b = _boxes(130, 5, 52)
    ub = numpy.arange(130) % 5 != 1
    space = numpy.stack([numpy.full((1, 5), -INF), numpy.full((1, 5), INF)], axis=1)
    pa, pb, _ = box_pairs(space, [True], b, ub, margin=TOL)
    want = ref.all_pairs(space, [True], b, ub, TOL)
    _same((pa, pb), want)
    thin = numpy.any(b[:, 1] - b[:, 0] <= TOL, axis=1)
    assert numpy.array_equal(pb, numpy.flatnonzero(ub & ~thin))


# ---- 4. row ranges, counts, overflow, determinism ------------------------------------------------------------------------------------------
def test_row_ranges_and_counts():
    a, b = _boxes(257, 5, 51), _boxes(130, 5, 52)
    ua, ub = numpy.arange(257) % 7 != 3, numpy.arange(130) % 5 != 1
    for fam_b in ((b, ub), (None, None)):
        full = box_pairs(a, ua, *fam_b, margin=TOL)
        parts = [box_pairs(a, ua, *fam_b, margin=TOL, rows=r) for r in ((0, 100), (100, 101), (101, 257))]
        assert numpy.array_equal(numpy.concatenate([p[0] for p in parts]), full[0])
        assert numpy.array_equal(numpy.concatenate([p[1] for p in parts]), full[1])
        assert sum(p[2]['tests'] for p in parts) == full[2]['tests'] and len(full[0]) > 1000
        counts, st = box_pairs(a, ua, *fam_b, margin=TOL, count_only=True)
        assert counts.dtype == numpy.int64 and numpy.array_equal(counts, numpy.bincount(full[0], minlength=257)) and st['pairs'] == len(full[0])
        counts, _ = box_pairs(a, ua, *fam_b, margin=TOL, rows=(100, 230), count_only=True)
        assert numpy.array_equal(counts, numpy.bincount(full[0], minlength=257)[100:230])
        empty = box_pairs(a, ua, *fam_b, margin=TOL, rows=(40, 40))
        assert len(empty[0]) == 0 and empty[2]['tests'] == 0


def test_a_list_that_does_not_fit_is_not_written():
    a, b = _boxes(257, 2, 21), _boxes(130, 2, 22)
    ua, ub = numpy.ones(257, dtype=bool), numpy.ones(130, dtype=bool)
    want = ref.all_pairs(a, ua, b, ub, TOL)
    n = len(want[0])
    pa, pb = numpy.full(n, -1, dtype=numpy.int64), numpy.full(n, -1, dtype=numpy.int64)
    total, out_a, out_b, _, st = _lib.box_pairs(a, ua, b, ub, TOL, 0, 257, n - 1, pair_a=pa, pair_b=pb)
    assert total == n and st['pairs'] == n and out_a is pa and numpy.all(pa == -1) and numpy.all(pb == -1)
    total, _, _, _, _ = _lib.box_pairs(a, ua, b, ub, TOL, 0, 257, 0)                    # the count-only call: null pointers
    assert total == n
    total, _, _, _, _ = _lib.box_pairs(a, ua, b, ub, TOL, 0, 257, n, pair_a=pa, pair_b=pb)
    assert total == n and numpy.array_equal(pa, want[0]) and numpy.array_equal(pb, want[1])
    got = box_pairs(a, ua, b, ub, margin=TOL, cap=n - 1)                              # the wrapper's retry
    _same(got, want)
    assert got[2]['calls'] == 2
    assert box_pairs(a, ua, b, ub, margin=TOL, cap=n)[2]['calls'] == 1


def test_two_calls_give_identical_bytes():
    a, b = _boxes(257, 16, 161), _boxes(130, 16, 162)
    ua, ub = numpy.arange(257) % 7 != 3, numpy.arange(130) % 5 != 1
    first, again = box_pairs(a, ua, b, ub, margin=TOL), box_pairs(a, ua, b, ub, margin=TOL)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and len(first[0]) > 1000
    polys = [ref.axis_rows(x) for x in a]
    off, ef = cases.csr(polys)
    k1, s1 = screen_pairs(off, ef, first[0], first[1] % 257, a, a)
    k2, s2 = screen_pairs(off, ef, first[0], first[1] % 257, a, a)
    assert k1.tobytes() == k2.tobytes() and {k: v for k, v in s1.items() if k != 'ms'} == {k: v for k, v in s2.items() if k != 'ms'}


# ---- 5. refusals of the library ------------------------------------------------------------------------------------------------------------
def test_library_refusals():
    a, ua = numpy.ascontiguousarray(_boxes(5, 2, 0)), numpy.ones(5, dtype=numpy.uint8)
    L = _lib.load()
    total, st = numpy.zeros(1, dtype=numpy.int64), numpy.zeros(3, dtype=numpy.int64)
    pa, pb = numpy.zeros(64, dtype=numpy.int64), numpy.zeros(64, dtype=numpy.int64)
    P = _lib._ptr
    # device, n_t, mode, n_a, box_a, usable_a, n_b, box_b, usable_b, margin, i0, i1, cap, pair_a, pair_b, row_count, total, stats, ms
    args = [0, 2, _lib.BOX_CROSS, 5, P(a), P(ua), 5, P(a), P(ua), TOL, 0, 5, 64, P(pa), P(pb), None, P(total), P(st), None]
    assert L.mpc_box_pairs(*args) == _lib.MPC_OK and total[0] == len(ref.all_pairs(a, ua, a, ua, TOL)[0])
    other = a.copy()
    for change, text in (({4: None}, 'missing array'), ({5: None}, 'missing array'), ({7: None}, 'missing array'), ({8: None}, 'missing array'),
                         ({16: None}, 'missing array'), ({13: None}, 'missing array'), ({14: None}, 'missing array'),
                         ({1: 0}, 'n_t must lie in 1..16'), ({1: 17}, 'n_t must lie in 1..16'), ({2: 2}, 'mode must be'),
                         ({3: 0}, 'a family has no box'), ({6: 0}, 'a family has no box'),
                         ({2: _lib.BOX_UPPER, 7: P(other)}, 'UPPER takes one family'), ({2: _lib.BOX_UPPER, 6: 4}, 'UPPER takes one family'),
                         ({10: -1}, 'row range'), ({11: 6}, 'row range'), ({10: 3, 11: 2}, 'row range'), ({12: -1}, 'cap must be >= 0'),
                         ({9: NAN}, 'margin must be finite'), ({9: INF}, 'margin must be finite')):
        broken = list(args)
        for k, v in change.items():
            broken[k] = v
        assert L.mpc_box_pairs(*broken) == _lib.MPC_ERR_INVALID, change
        assert text.encode() in L.mpc_last_error(None), (change, L.mpc_last_error(None))
    upper = list(args)
    upper[2], upper[6], upper[7], upper[8] = _lib.BOX_UPPER, 0, None, None                     # UPPER with family b left out
    assert L.mpc_box_pairs(*upper) == _lib.MPC_OK and total[0] == len(ref.all_pairs(a, ua, margin=TOL)[0])
    # through the wrappers: MpcError with the library's message
    with pytest.raises(_lib.MpcError, match='margin must be finite'):
        _lib.box_pairs(a, ua, None, None, NAN, 0, 5, 0)
    with pytest.raises(_lib.MpcError, match='row range'):
        _lib.box_pairs(a, ua, a, ua, TOL, 2, 9, 0)
    with pytest.raises(_lib.MpcError, match=r'n_t must lie in 1\.\.16'):
        _lib.box_pairs(numpy.zeros((2, 2, 17)), [1, 1], None, None, TOL, 0, 2, 0)
    polys = [ref.axis_rows(x) for x in a]
    off, ef = cases.csr(polys)
    keep, st = _lib.pair_screen(off, ef, [0, 1], [1, 2], a, a, 3)
    assert keep.dtype == numpy.uint8 and st['pairs'] == 2
    bad_rows = ef.copy()
    bad_rows[1, 1:] *= 2.0
    for kw, text in ((dict(pa=[0, 5]), 'out of range'), (dict(pb=[-1, 1]), 'out of range'), (dict(sides=0), 'sides must be'), (dict(sides=4), 'sides must be'),
                     (dict(box_a=None), 'missing array'), (dict(box_b=None), 'missing array'), (dict(ef=bad_rows), 'unit normals')):
        with pytest.raises(_lib.MpcError, match=text):
            _lib.pair_screen(off, kw.get('ef', ef), kw.get('pa', [0, 1]), kw.get('pb', [1, 2]), kw.get('box_a', a), kw.get('box_b', a), kw.get('sides', 3))
    assert _lib.pair_screen(off, ef, [0, 1], [1, 2], None, a, _lib.SCREEN_ROWS_B)[1]['pairs'] == 2      # the box of the other side may be left out
    assert _lib.pair_screen(off, ef, [], [], None, None, 3)[1]['pairs'] == 0                            # no candidate: nothing else is looked at


# ---- 6. the screen ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_t', [1, 5, 16])
def test_the_screen_on_dyadic_boxes_equals_the_reference(n_t):
    """axis-aligned rows with dyadic offsets against dyadic boxes: every s - o is exact, the masks are equal"""
    R = 70
    regions, boxes = _boxes(R, n_t, 10 * n_t + 7), _boxes(R, n_t, 10 * n_t + 8)
    regions = numpy.stack([regions[:, 0], numpy.maximum(regions[:, 1], regions[:, 0])], axis=1)
    polys = [ref.axis_rows(x) for x in regions]
    off, ef = cases.csr(polys)
    i, j = numpy.divmod(numpy.arange(R * R), R)
    for sides in ('a', 'b', 'both'):
        keep, st = screen_pairs(off, ef, i, j, boxes, regions, sides=sides)
        want = ref.screen(polys, i, j, boxes, regions, sides)
        assert keep.dtype == bool and numpy.array_equal(keep, want), sides
        assert st['pairs'] == R * R and st['dropped'] == int((~want).sum()) and 0 < st['dropped'] < R * R
    # both sides against the regions' own boxes: a pair is kept iff the two boxes share a point
    keep, _ = screen_pairs(off, ef, i, j, regions, regions)
    d = ref.overlap_matrix(regions, regions)
    assert numpy.array_equal(keep.reshape(R, R), numpy.all(d >= 0.0, axis=2))


@functools.lru_cache(maxsize=None)
def _bsp(n):
    """the BSP set of compare_cases (padded to 256 rows per region at n = 16) in one table with the device's points and boxes"""
    case = cases.padded(n) if n == 16 else cases.synthetic(n)
    polys, laws, n_a = cases.table(case)
    off, ef = cases.csr(polys)
    xs, box, status, _ = _lib.merge_regions(off, ef)
    assert numpy.all(status == 0)
    return polys, laws, n_a, off, ef, xs, box


@pytest.mark.parametrize('n', [2, 5, 16])
def test_the_screen_keeps_every_meeting_pair_of_the_bsp_sets(n):
    polys, laws, n_a, off, ef, xs, box = _bsp(n)
    R = len(polys)
    use = numpy.ones(R, dtype=bool)
    pa, pb, _ = box_pairs(box[:n_a], use[:n_a], box[n_a:], use[n_a:], margin=LP_TOL)
    _same((pa, pb), cmp.cross_box_pairs(box[:n_a], use[:n_a], box[n_a:], use[n_a:], LP_TOL))
    pb = pb + n_a
    res = cmp.law_gap_pairs(off, ef, laws, pa, pb, tol=LP_TOL, xs=xs)
    meets = res['radius'] > LP_TOL
    assert meets.sum() == cases.SHAPES[n][3]
    excess_a = numpy.array([ref.least_excess(polys[i], box[j]) for i, j in zip(pa.tolist(), pb.tolist())])
    excess_b = numpy.array([ref.least_excess(polys[j], box[i]) for i, j in zip(pa.tolist(), pb.tolist())])
    for sides in ('both', 'a', 'b'):
        keep, st = screen_pairs(off, ef, pa, pb, box, box, sides=sides)
        assert numpy.all(keep[meets]), (sides, numpy.flatnonzero(meets & ~keep))
        excess = {'a': excess_a, 'b': excess_b, 'both': numpy.maximum(excess_a, excess_b)}[sides]
        assert not numpy.any(keep[excess > 1e-9]), sides                    # what the reference drops clearly is dropped
        assert numpy.all(keep[excess < -1e-9]), sides                       # and what it keeps clearly is kept
        assert st['dropped'] == int((~keep).sum())


@pytest.mark.parametrize('n', [2, 5, 16])
def test_the_one_sided_screen_under_identity_maps(n):
    """transition_pairs with Phi = I, phi = 0: the image of a region is the region, T_ij = R_i n R_j"""
    polys, _, _, off, ef, _, _ = _bsp(n)
    R = len(polys)
    Phi, phi = numpy.tile(numpy.eye(n), (R, 1, 1)), numpy.zeros((R, n))
    plain = tr.transition_pairs(off, ef, Phi, phi, n, tol=LP_TOL, full_radius=True)
    swept = tr.transition_pairs(off, ef, Phi, phi, n, tol=LP_TOL, full_radius=True, sweep='device')
    for key in ('i', 'j', 'radius', 'status', 'witness'):
        assert plain[key].tobytes() == swept[key].tobytes(), key
    kept = tr.transition_pairs(off, ef, Phi, phi, n, tol=LP_TOL, full_radius=True, sweep='device', screen='rows')
    code = lambda r: r['i'] * R + r['j']
    where = numpy.searchsorted(code(plain), code(kept))
    assert numpy.array_equal(code(plain)[where], code(kept))                # a subset of the candidates, in order
    edges = plain['status'] != tr.NO_EDGE
    assert numpy.all(numpy.isin(code(plain)[edges], code(kept)))            # with every edge
    for key in ('radius', 'status', 'witness'):
        assert plain[key][where].tobytes() == kept[key].tobytes(), key
    st = kept['stats']
    assert st['box_candidates'] == len(plain['i']) and st['candidates'] == len(kept['i']) == st['box_candidates'] - st['screened']
    assert st['edges'] == plain['stats']['edges'] >= R
    # the screen runs on the widened image boxes (transition.screen_box): the reference on the same boxes
    assert numpy.all(kept['screen_box'][:, 0] < plain['image_box'][:, 0]) and numpy.all(kept['screen_box'][:, 1] > plain['image_box'][:, 1])
    assert 'screen_box' not in plain and 'screen_box' not in swept
    excess = numpy.array([ref.least_excess(polys[j], kept['screen_box'][i]) for i, j in zip(plain['i'].tolist(), plain['j'].tolist())])
    gone = ~numpy.isin(code(plain), code(kept))
    assert numpy.all(gone[excess > 1e-9]) and not numpy.any(gone[excess < -1e-9])


# ---- 7. wiring: sweep= and screen= of the public calls ---------------------------------------------------------------------------------------
def _counters(stats):
    return {k: v for k, v in stats.items() if not k.endswith('_ms')}


@functools.lru_cache(maxsize=None)
def _double_integrator(horizon):
    d = pg.double_integrator_data(horizon=horizon)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        prog = MPQP_Program(d['A'], d['b'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], d['F'], equality_indices=d.get('equality_indices'))
        sol = solve_mpqp(prog, mpqp_algorithm.combinatorial)
    plain = Solution(sol.program, sol.critical_regions, is_overlapping=False, point_location_tolerance=sol.point_location_tolerance)
    plain.is_complete = sol.is_complete
    return plain


def _bsp_solutions(n):
    """the two partitions of synthetic(n) as solutions without a program: regions E theta <= f with the laws of the set"""
    case = cases.synthetic(n)
    out = []
    for polys, laws in ((case['polys_a'], case['laws_a']), (case['polys_b'], case['laws_b'])):
        regs = [CriticalRegion(l[:, 1:].copy(), l[:, :1].copy(), numpy.zeros((0, n)), numpy.zeros((0, 1)), p[:, 1:].copy(), p[:, :1].copy(), [k])
                for k, (p, l) in enumerate(zip(polys, laws))]
        out.append(Solution(None, regs, is_overlapping=False))
    return out


LAW_GAP_ARRAYS = ('i', 'j', 'radius', 'gap', 'row', 'witness', 'flag', 'usable_a', 'usable_b')


def _check_compare(a, b, **kw):
    host = a.compare(b, **kw)
    dev = a.compare(b, sweep='device', **kw)
    for key in LAW_GAP_ARRAYS:
        assert getattr(host, key).tobytes() == getattr(dev, key).tobytes(), key
    assert _counters(host.stats) == _counters(dev.stats) and 'sweep_kernel_ms' in dev.stats and dev.stats['sweep_ms'] > 0.0
    for sweep in ('device', 'host'):
        kept = a.compare(b, sweep=sweep, screen='rows', **kw)
        code = lambda g: g.i * host.n_b + g.j
        where = numpy.searchsorted(code(host), code(kept))
        assert numpy.array_equal(code(host)[where], code(kept))             # a subset of the candidates, in order
        assert numpy.all(numpy.isin(code(host)[host.meets], code(kept)))    # with every meeting pair
        for key in ('radius', 'gap', 'row', 'witness', 'flag'):
            assert getattr(host, key)[where].tobytes() == getattr(kept, key).tobytes(), (sweep, key)
        assert kept.max_gap == host.max_gap and kept.argmax >= 0 and code(kept)[kept.argmax] == code(host)[host.argmax]
        assert numpy.array_equal(kept.unmatched_a, host.unmatched_a) and numpy.array_equal(kept.unmatched_b, host.unmatched_b)
        st = kept.stats
        assert st['box_candidates'] == len(host.i) and st['candidates'] == len(kept.i) == st['pairs'] == st['box_candidates'] - st['screened']
        assert st['meets'] == host.stats['meets'] and st['screen_ms'] > 0.0
    return host, kept


def test_compare_with_the_device_sweep_and_the_screen():
    a, b = _double_integrator(2), _double_integrator(3)
    _check_compare(b, b)
    _check_compare(a, b, outputs=[0])
    sa, sb = _bsp_solutions(3)
    host, kept = _check_compare(sa, sb)
    assert host.stats['meets'] == cases.SHAPES[3][3] and kept.stats['screened'] > 0


def test_transition_graph_with_the_device_sweep_and_the_screen():
    sol, plant = _double_integrator(3), pg.double_integrator_plant(3)
    host = sol.transition_graph(plant['A'], plant['B'], plant['inputs'], full_radius=True)
    for kw in (dict(sweep='device'), dict(sweep='device', screen='rows'), dict(sweep='host', screen='rows')):
        g = sol.transition_graph(plant['A'], plant['B'], plant['inputs'], full_radius=True, **kw)
        for key in ('indptr', 'indices', 'radius', 'status', 'witness', 'region_status'):
            assert getattr(host, key).tobytes() == getattr(g, key).tobytes(), (kw, key)
        if 'screen' in kw:
            assert g.stats['box_candidates'] == host.stats['candidates'] == g.stats['candidates'] + g.stats['screened']
            assert g.stats['edges'] == host.stats['edges']
        else:
            assert _counters(host.stats) == _counters(g.stats)
    assert len(host.indices) >= len(sol)


def test_remove_overlaps_with_the_device_sweep_and_the_screen():
    from test_gpu_overlap import _solved
    prog, sol, red = _solved('mplp')
    for kw in (dict(sweep='device'), dict(sweep='device', screen='rows'), dict(sweep='host', screen='rows')):
        other = sol.remove_overlaps(**kw)
        assert len(other) == len(red)
        for p, q in zip(red.critical_regions, other.critical_regions):
            assert p.source == q.source and p.E.tobytes() == q.E.tobytes() and p.f.tobytes() == q.f.tobytes()
        assert numpy.array_equal(other.overlap_info['sources'], red.overlap_info['sources'])
        assert other.overlap_info['vanished'] == red.overlap_info['vanished']
        if 'screen' not in kw:
            assert other.overlap_info['verdict_counts'] == red.overlap_info['verdict_counts']
            assert _counters(other.overlap_info['stats']) == _counters(red.overlap_info['stats'])
    # one BSP partition against itself shifted: overlapping cells with affine values, through the arrays
    case = cases.synthetic(2)
    polys = case['polys_a'] + case['polys_b']
    off, ef = cases.csr(polys)
    rng = numpy.random.default_rng(9)
    g, h = rng.normal(size=(len(polys), 2)), rng.normal(size=len(polys))
    host = overlap.partition_by_value(off, ef, g, h, 2, tol=LP_TOL)
    dev = overlap.partition_by_value(off, ef, g, h, 2, tol=LP_TOL, sweep='device')
    for key in ('i', 'j', 'verdict', 'radius', 'd_min', 'd_max'):
        assert host.pairs[key].tobytes() == dev.pairs[key].tobytes(), key
    kept = overlap.partition_by_value(off, ef, g, h, 2, tol=LP_TOL, sweep='device', screen='rows')
    assert kept.stats['box_candidates'] == len(host.pairs['i']) and kept.stats['screened'] > 0
    R = len(polys)
    code = lambda p: p['i'] * R + p['j']
    where = numpy.searchsorted(code(host.pairs), code(kept.pairs))
    assert numpy.array_equal(code(host.pairs)[where], code(kept.pairs))
    assert numpy.all(numpy.isin(code(host.pairs)[host.pairs['verdict'] != overlap.DISJOINT], code(kept.pairs)))
    for key in ('verdict', 'radius', 'd_min', 'd_max'):
        assert host.pairs[key][where].tobytes() == kept.pairs[key].tobytes(), key
    assert numpy.array_equal(host.sources, dev.sources) and numpy.array_equal(host.sources, kept.sources)
    for p, q, r in zip(host.pieces, dev.pieces, kept.pieces):
        assert (p is None) == (q is None) == (r is None) and (p is None or (p.tobytes() == q.tobytes() == r.tobytes()))


# ---- 8. the keys of stats, per call and per setting -----------------------------------------------------------------------------------------
def _settings():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('sweep_bench', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'sweep_bench.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.SETTINGS


SWEEP_KEYS = {('host', 'none'): set(), ('device', 'none'): {'sweep_kernel_ms'},
              ('device', 'rows'): {'sweep_kernel_ms', 'box_candidates', 'screened', 'screen_kernel_ms', 'screen_ms'},
              ('host', 'rows'): {'box_candidates', 'screened', 'screen_kernel_ms', 'screen_ms'}}
OVERLAP_KEYS = {'regions_before', 'candidate_pairs', 'rounds', 'work_items', 'max_item_rows', 'lps', 'pivots', 'wide', 'device_ms', 'regions_after', 'wall_ms'}
GRAPH_KEYS = {'box_ms', 'pair_ms', 'sweep_ms', 'candidates', 'lps', 'pivots', 'capped', 'edges', 'box_lps', 'box_pivots', 'wall_ms'}
COMPARE_KEYS = {'pairs', 'meets', 'constant_rows', 'lps', 'pivots', 'wide', 'pair_ms', 'device_ms', 'candidates', 'box_pairs', 'sweep_ms', 'wall_ms'}


def test_the_keys_of_stats_in_the_four_settings():
    """The twelve key sets as they were when every call had its own candidate stage: remove_overlaps reports sweep_ms only with the device
    sweep or the screen, the other two always.  And the results of the four settings are the same bytes (compare: on the meeting pairs,
    the only ones every setting lists; all pairs between the two settings with and the two without the screen)."""
    settings = _settings()
    assert set(settings) == set(SWEEP_KEYS) and len(settings) == 4
    from test_gpu_overlap import _solved
    _, overlapping, _ = _solved('mplp')
    sol, plant = _double_integrator(2), pg.double_integrator_plant(2)
    reduced, graphs, gaps = {}, {}, {}
    for sweep, screen in settings:
        kw = dict(sweep=sweep, screen=screen)
        reduced[sweep, screen] = overlapping.remove_overlaps(**kw)
        graphs[sweep, screen] = sol.transition_graph(plant['A'], plant['B'], plant['inputs'], **kw)
        gaps[sweep, screen] = sol.compare(sol, **kw)
        extra = SWEEP_KEYS[sweep, screen]
        assert set(reduced[sweep, screen].overlap_info['stats']) == OVERLAP_KEYS | extra | ({'sweep_ms'} if extra else set()), kw
        assert set(graphs[sweep, screen].stats) == GRAPH_KEYS | extra, kw
        assert set(gaps[sweep, screen].stats) == COMPARE_KEYS | extra, kw
    first = settings[0]
    for s in settings[1:]:
        for key in ('indptr', 'indices', 'radius', 'status', 'witness', 'region_status'):
            assert getattr(graphs[first], key).tobytes() == getattr(graphs[s], key).tobytes(), (s, key)
        assert reduced[first].overlap_info['sources'].tobytes() == reduced[s].overlap_info['sources'].tobytes(), s
        assert len(reduced[first]) == len(reduced[s])
        for p, q in zip(reduced[first].critical_regions, reduced[s].critical_regions):
            assert p.E.tobytes() == q.E.tobytes() and p.f.tobytes() == q.f.tobytes(), s
        a, b = gaps[first], gaps[s]
        for key in ('i', 'j', 'radius', 'gap', 'row', 'witness', 'flag'):
            assert getattr(a, key)[a.meets].tobytes() == getattr(b, key)[b.meets].tobytes(), (s, key)
    for a, b in ((gaps['host', 'none'], gaps['device', 'none']), (gaps['host', 'rows'], gaps['device', 'rows'])):
        for key in LAW_GAP_ARRAYS:
            assert getattr(a, key).tobytes() == getattr(b, key).tobytes(), key
