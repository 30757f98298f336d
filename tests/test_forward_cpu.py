"""The host side of Solution.reach_cells without a device: the CPU reference on the hand cases, locate / state_at /
itinerary on hand-made cells, every ValueError of the arrays form, the ordering rules."""
import numpy
import pytest

import exit_cases as xc
import forward_cases as fc
import forward_reference as fref
from ppopt_amd import reach


def _cells(cells):
    """a ForwardCells of reference cells"""
    off, rows = xc.csr([c['rows'] for c in cells])
    n = len(cells)
    n_t = rows.shape[1] - 1
    return reach.ForwardCells(n_regions=1 + max(c['region'] for c in cells), cell_off=off, cell_rows=rows,
                              region=numpy.asarray([c['region'] for c in cells], dtype=numpy.int64),
                              step=numpy.asarray([c['step'] for c in cells], dtype=numpy.int64),
                              parent=numpy.asarray([c['parent'] for c in cells], dtype=numpy.int64), G=numpy.asarray([c['G'] for c in cells]),
                              g=numpy.asarray([c['g'] for c in cells]), wide=numpy.zeros(n, dtype=bool), point=numpy.zeros((n, n_t)),
                              steps=max(c['step'] for c in cells))


def test_reference_on_the_tent_map_by_hand():
    """forward_cases.tent_cells: the dyadic intervals in order of lineage, G = +-2^k, dyadic g; every number exact"""
    polys, Phi, phi, succ = fc.tent_map()
    steps = 4
    cells, items, status = fref.forward_reference(polys, Phi, phi, succ, list(enumerate(polys)), fc.TOL, steps)
    want = fc.tent_cells(steps)
    # (every item is a knife item by definition: a row of Q beside its pulled-back copy gives a radius of exactly 0, within the band of tol)
    assert status == 'DONE' and len(cells) == len(want) == sum(2 ** (k + 1) for k in range(steps + 1))
    iv = xc.intervals([(c['region'], c['rows']) for c in cells])
    for c, w, (_, got_lo, got_hi) in zip(cells, want, iv):
        lo, hi, G, g, region, parent = w
        assert (got_lo, got_hi) == (lo, hi) and c['G'][0, 0] == G and c['g'][0] == g and c['region'] == region and c['parent'] == parent
        assert abs(G) == 2.0 ** c['step'] and hi - lo == 2.0 ** -(c['step'] + 1) and len(c['rows']) == 2
        assert c['step'] == 0 or numpy.array_equal(c['rows'], fc.tent_rows(w))
    for k in range(steps + 1):      # the cells of a step tile [0, 1]
        at = sorted((lo, hi) for (_, lo, hi), c in zip(iv, cells) if c['step'] == k)
        assert at[0][0] == 0.0 and at[-1][1] == 1.0 and all(a[1] == b[0] for a, b in zip(at, at[1:]))
    # the items: by parent cell, then by region ascending; two per parent, each a cell after 1 + 4 LPs with two unbounded runs (in 1-D the
    # run beyond an interval's only bound of a kind is unbounded: the two rows of Q go first, as redundant; the pulled-back pair is alone then)
    assert [(i['parent'], i['region']) for i in items] == [(c, j) for c in range(len(cells) - 2 ** (steps + 1)) for j in (0, 1)]
    assert all(i['outcome'] == 'cell' and i['lps'] == 5 and i['wide'] == 2 for i in items) and not any(c['wide'] for c in cells)


def test_reference_on_constant_rows_and_a_zero_map():
    """exit_cases.constant_rows from step 0 = the two squares: (A, B) drops B's rows in y (beta = 1/2) and keeps 0 <= x <= 1: the cell is A
    whole, with y <= 1 and -y <= 0 of A and the pulled-back x <= 1 and -x <= 0 (A's own two are met first and are redundant beside their
    copies), after 1 + 4 + 2 LPs; (B, A) and (B, B) meet the constant row -y <= 0 with beta = -1/2: empty, no LP.  At step 2 the cell's
    next map is Phi_B Phi_A = diag(1, 0), s = (2, -1/2): empty again, so the status is EMPTY after one step.
    Phi = 0 on the unit square with theta+ = (1/2, 1/2): every pulled-back row is constant with beta = 1/2, the child is the parent whole
    with G = 0, g = (1/2, 1/2), at every step."""
    polys, Phi, phi, succ = xc.constant_rows()
    cells, items, status = fref.forward_reference(polys, Phi, phi, succ, list(enumerate(polys)), fc.TOL, 3)
    assert status == 'EMPTY' and [c['step'] for c in cells] == [0, 0, 1] and [(i['parent'], i['region'], i['outcome'], i['lps']) for i in items] == \
        [(0, 1, 'cell', 7), (1, 0, 'empty', 0), (1, 1, 'empty', 0), (2, 0, 'empty', 0), (2, 1, 'empty', 0)]
    assert numpy.array_equal(cells[2]['rows'], numpy.array([[1.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 1.0, 0.0], [0.0, -1.0, 0.0]]))
    assert numpy.array_equal(cells[2]['G'], Phi[0]) and numpy.array_equal(cells[2]['g'], phi[0]) and cells[2]['region'] == 1
    S = xc.box_rows([0, 0], [1, 1])
    cells, items, status = fref.forward_reference([S], numpy.zeros((1, 2, 2)), numpy.array([[0.5, 0.5]]), [[0]], [(0, S)], fc.TOL, 3)
    assert status == 'DONE' and len(cells) == 4 and all(i['lps'] == 5 for i in items)
    for c in cells[1:]:
        assert numpy.array_equal(c['rows'], S) and not c['G'].any() and c['g'].tolist() == [0.5, 0.5]


def test_recorded_reference_runs_are_the_reference():
    """tests/golden/forward_set_*.npz (python tests/forward_reference.py) hold the reference's runs on exit_cases.SETS, which the GPU file
    compares against without spending its time on HiGHS: the smallest one again from scratch, every recorded bit; of the others the first
    step; and the knife counts that DESIGN §3.25 lists"""
    import exit_reference as xref
    counts = []
    for case in fc.SETS:
        z = numpy.load(fref.golden_path(case))
        cells, items, status = fref.unpack(z)
        counts.append((len(items), sum(i['knife'] for i in items)))
        polys, Phi, phi = xc.synthetic_set(*case)
        if case[0] == 5:
            again = fref.set_reference(case, fc.SET_TOL, fc.SET_STEPS)
            # every array bit for bit, the maps included (explicit loops over IEEE doubles); the rows, which pass through a matrix
            # product of the BLAS at hand, within 1e-12
            assert sorted(again) == sorted(z.files) and all(numpy.asarray(again[k]).tobytes() == z[k].tobytes() for k in again if k != 'cell_rows')
            assert again['cell_rows'].shape == z['cell_rows'].shape and numpy.all(numpy.abs(again['cell_rows'] - z['cell_rows']) <= 1e-12)
        else:
            succ = [z['succ_idx'][z['succ_off'][i]:z['succ_off'][i + 1]].tolist() for i in range(len(polys))]
            first, first_items, _ = fref.forward_reference(polys, Phi, phi, succ, list(enumerate(polys)), fc.SET_TOL, 1)
            assert len(first) == sum(c['step'] <= 1 for c in cells) and len(first_items) == sum(i['step'] == 1 for i in items)
            for a, b in zip(first, cells):
                assert a['lineage'] == b['lineage'] and a['rows'].shape == b['rows'].shape and numpy.all(numpy.abs(a['rows'] - b['rows']) <= 1e-12)
                assert numpy.array_equal(a['G'], b['G']) and numpy.array_equal(a['g'], b['g'])
        assert status == 'DONE' and max(c['step'] for c in cells) == fc.SET_STEPS and len(cells) > len(polys)
    assert counts == [(3293, 0), (670, 0), (89, 0)] and all(k <= fc.KNIFE_CAP * n for n, k in counts)


def test_next_map_sums_ascending_from_zero():
    """((0 + a_0 b_0) + a_1 b_1) + a_2 b_2: with (1e16, 1, -1e16) the 1 is lost, in any other order it is not"""
    Phi_i = numpy.array([[1e16, 1.0, -1e16], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    P, s = fref.next_map(Phi_i, numpy.array([0.25, 0.0, 0.0]), numpy.ones((3, 3)), numpy.ones(3))
    assert P[0].tolist() == [0.0, 0.0, 0.0] and s[0] == 0.25 and (Phi_i @ numpy.ones(3))[0] in (0.0, 1.0, 2.0)
    rng = numpy.random.default_rng(0)
    A, G, g, p = rng.integers(-8, 9, (4, 4)) / 4.0, rng.integers(-8, 9, (4, 4)) / 8.0, rng.integers(-8, 9, 4) / 2.0, rng.integers(-8, 9, 4) / 16.0
    P, s = fref.next_map(A, p, G, g)
    assert numpy.array_equal(P, A @ G) and numpy.array_equal(s, A @ g + p)      # dyadic: exact in any order


def test_locate_state_at_and_itinerary_on_hand_made_cells():
    polys, Phi, phi, succ = fc.tent_map()
    cells, _, _ = fref.forward_reference(polys, Phi, phi, succ, list(enumerate(polys)), fc.TOL, 3)
    fw = _cells(cells)
    assert len(fw) == 30 and fw.cells_at(0).tolist() == [0, 1] and fw.cells_at(2).tolist() == list(range(6, 14)) and fw.cells_at(9).tolist() == []
    th = numpy.array([[0.3], [0.8], [0.5], [1.5], [-0.1], [0.0], [1.0]])
    tent = lambda x: numpy.where(x <= 0.5, 2.0 * x, 2.0 - 2.0 * x)
    x = th.copy()
    for k in range(4):
        c = fw.locate(th, k)
        assert (c[[3, 4]] == -1).all() and (c[[0, 1, 2, 5, 6]] >= 0).all() and numpy.all(fw.step[c[c >= 0]] == k)
        inside = c >= 0
        # the cell's region is the region of the state at step k (0.5 lies in both: the first cell that holds the point)
        assert numpy.all((x[inside, 0] <= 0.5) == (fw.region[c[inside]] == 0) | (x[inside, 0] == 0.5))
        got = fw.state_at(th, k)
        assert numpy.array_equal(got[inside], x[inside]) and numpy.all(numpy.isnan(got[~inside]))
        x = tent(x)
    assert fw.locate(numpy.array([0.3]), 0).tolist() == [0]                               # one point as a vector
    assert fw.locate(numpy.array([[1.0 + 1e-9]]), 1).tolist() == [-1] and fw.locate(numpy.array([[1.0 + 1e-9]]), 1, tol=1e-8).tolist() == [4]
    # 0.3 -> 0.6 -> 0.8 -> 0.4: the regions 0, 1, 1, 0
    c = int(fw.locate(numpy.array([[0.3]]), 3)[0])
    assert fw.itinerary(c) == [0, 1, 1, 0] and fw.itinerary(0) == [0] and cells[c]['lineage'] == (0, 1, 1, 0)
    for bad in (-1, 30):
        with pytest.raises(ValueError, match='itinerary'):
            fw.itinerary(bad)
    with pytest.raises(ValueError, match='thetas'):
        fw.locate(numpy.zeros((2, 2)), 0)
    with pytest.raises(ValueError, match='thetas'):
        fw.state_at(numpy.zeros((2, 3, 1)), 0)
    assert fw.roots().tolist() == [0, 1] + [c['lineage'][0] for c in cells[2:]]
    # images: cond(G) = 1 in 1-D: every image is a whole region
    for k in range(4):
        for rows, c in zip(fw.images(k), fw.cells_at(k)):
            (_, lo, hi), = xc.intervals([(0, rows)])
            assert (lo, hi) == ((0.0, 0.5) if fw.region[c] == 0 else (0.5, 1.0))
    flat = _cells([dict(cells[0], G=numpy.zeros((1, 1)))])
    assert flat.images(0) == [None]


def _base():
    polys, Phi, phi, succ = fc.tent_map()
    off, ef = xc.csr(polys)
    return dict(row_off=off, ef_rows=ef, Phi=Phi, phi=phi, n_t=1, successors=succ, cell_off=off, cell_rows=ef, cell_region=[0, 1], tol=1e-8,
                max_steps=4, max_cells=64)


def test_every_value_error_comes_before_the_library(monkeypatch):
    from ppopt_amd import _lib
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('the library was touched'))
    base = _base()
    off, ef, Phi, phi = base['row_off'], base['ef_rows'], base['Phi'], base['phi']
    big = numpy.tile(xc.box_rows([0], [1]), (129, 1))
    for kw, text in (({'n_t': 0}, 'outside 1..16'), ({'n_t': 17}, 'outside 1..16'), ({'tol': -1.0}, 'tol'), ({'tol': numpy.nan}, 'tol'),
                     ({'max_steps': -1}, 'max_steps'), ({'max_cells': 0}, 'max_cells'), ({'max_rows_total': 0}, 'max_rows_total'),
                     ({'row_off': off[1:]}, 'must describe'), ({'Phi': Phi[:1]}, 'must describe'), ({'phi': phi[:, :0]}, 'must describe'),
                     ({'row_off': [0, 0, 4]}, '1..256 rows'), ({'row_off': [0, 258], 'ef_rows': big, 'Phi': Phi[:1], 'phi': phi[:1]}, '1..256 rows'),
                     ({'ef_rows': numpy.full_like(ef, numpy.inf)}, 'finite'), ({'Phi': Phi * numpy.nan}, 'finite'), ({'successors': [[1]]}, 'one index list'),
                     ({'successors': [[2], []]}, 'must name polytopes'), ({'successors': [[-1], []]}, 'must name polytopes'),
                     ({'cell_off': off[:-1]}, 'cell_off'), ({'cell_region': [0]}, 'cell_off'), ({'cell_off': [0, 0, 4]}, 'every cell needs'),
                     ({'cell_off': [0, 258], 'cell_rows': big, 'cell_region': [0], 'max_rows_total': 1000}, 'every cell needs'),
                     ({'cell_region': [0, 2]}, 'cell_region'), ({'cell_region': [-1, 1]}, 'cell_region'),
                     ({'cell_rows': ef * numpy.nan}, 'cell rows must be finite'), ({'max_cells': 1}, 'step 0'), ({'max_rows_total': 3}, 'step 0'),
                     ({'cell_point': numpy.zeros((3, 1))}, 'cell_point'), ({'cell_point': numpy.full((2, 1), numpy.nan)}, 'cell_point')):
        with pytest.raises(ValueError, match=text):
            reach.forward_cells(**dict(base, **kw))
    # max_steps = 0 and an empty step 0 need no library either
    got = reach.forward_cells(**dict(base, max_steps=0))
    assert len(got) == 2 and got.status == 'DONE' and got.steps == 0 and got.locate(numpy.array([[0.2], [0.7], [2.0]]), 0).tolist() == [0, 1, -1]
    assert numpy.array_equal(got.G, numpy.ones((2, 1, 1))) and not got.g.any() and got.stats['cells_per_step'] == [2]
    none = reach.forward_cells(**dict(base, cell_off=[0], cell_rows=numpy.zeros((0, 2)), cell_region=[]))
    assert len(none) == 0 and none.status == 'EMPTY' and none.steps == 0 and none.locate(numpy.array([[0.2]]), 0).tolist() == [-1]


def test_successor_lists_go_to_the_library_ascending_and_once(monkeypatch):
    """the arrays form hands the library every successor list ascending, once each, and the cells of step 0 with a point each"""
    from ppopt_amd import _lib
    seen = {}

    def fake_forward(off, ef, Phi, phi, succ_off, succ_idx, coff, crow, creg, cpt, tol, max_steps, max_cells, max_rows, device=0):
        seen.update(succ_off=numpy.asarray(succ_off).tolist(), succ_idx=numpy.asarray(succ_idx).tolist(), cpt=numpy.asarray(cpt).copy())
        n = len(creg)
        return {'cell_off': coff, 'cell_rows': crow, 'region': numpy.asarray(creg), 'step': numpy.zeros(n, dtype=numpy.int64),
                'parent': numpy.full(n, -1), 'wide': numpy.zeros(n, dtype=bool), 'point': cpt, 'G': numpy.ones((n, 1, 1)), 'g': numpy.zeros((n, 1)),
                'status': 1, 'steps': 0, 'cells_per_step': numpy.asarray([n]), 'step_ms': numpy.zeros(max_steps),
                'stats': dict(items=0, cells=0, empty=0, lps=0, pivots=0, wide=0, ms=0.0)}

    monkeypatch.setattr(_lib, 'forward_cells', fake_forward)
    monkeypatch.setattr(_lib, 'merge_regions', lambda off, ef, device=0: (numpy.array([[0.25], [numpy.nan]]), None, None, {'ms': 0.0}))
    got = reach.forward_cells(**dict(_base(), successors=[[1, 0, 1], numpy.array([1])]))
    assert seen['succ_off'] == [0, 2, 3] and seen['succ_idx'] == [0, 1, 1] and seen['cpt'].tolist() == [[0.25], [0.0]] and got.status == 'EMPTY'
    reach.forward_cells(**dict(_base(), cell_point=[[0.1], [0.9]]))
    assert seen['cpt'].tolist() == [[0.1], [0.9]]
