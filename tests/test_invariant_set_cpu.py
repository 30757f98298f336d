"""The host side of Solution.invariant_set without a device: the CPU reference on the hand cases, exit_step / contains on
hand-made cells, every ValueError of the arrays form, the ordering rules."""
import numpy
import pytest

import exit_cases as xc
import exit_reference as xref
import invariant_cases as ic
import invariant_reference as iref
from ppopt_amd import invariant_set as inv


def test_reference_on_the_one_d_hand_case():
    polys, Phi, phi, succ = xc.one_d_loop(4)
    pieces, knife = xref.exit_reference(polys, Phi, phi, succ, 1e-3)
    assert not knife and numpy.allclose([p[1:] for p in xc.intervals([(s, r) for s, r, _, _ in pieces])],
                                        [p[1:] for p in xc.intervals(ic.one_d_cells0())], rtol=0, atol=1e-12)
    cells, items, conv = iref.backward_reference(polys, Phi, phi, ic.predecessors_of(succ), ic.one_d_cells0(), 1e-3)
    steps, small_until = ic.one_d_steps(1e-3)
    assert (steps, small_until) == (3, 2) and ic.one_d_steps(1e-8) == (12, 10)
    assert conv and max(c['step'] for c in cells) == steps and not any(i['knife'] for i in items)
    assert [sum(c['step'] == k for c in cells) for k in range(steps + 1)] == [4, 4, 4, 2]
    iv = xc.intervals([(c['source'], c['rows']) for c in cells])
    want1 = [(-3 / 16, -1 / 16), (3 / 64, 1 / 16), (-1 / 16, -3 / 64), (1 / 16, 3 / 16)]
    for k in range(1, steps + 1):
        got = [p[1:] for p, c in zip(iv, cells) if c['step'] == k]
        want = [(a / 4 ** (k - 1), b / 4 ** (k - 1)) for a, b in want1] if k <= small_until else [(a / 16, b / 16) for a, b in (want1[0], want1[3])]
        assert numpy.allclose(got, want, rtol=0, atol=1e-12), k
    assert all(c['source'] == 1 and cells[c['parent']]['step'] == c['step'] - 1 for c in cells if c['step'])
    # the items of a step: by parent cell, then by region ascending; one region (M) precedes every region here
    assert [(i['parent'], i['region']) for i in items if i['step'] == 1] == [(0, 1), (1, 1), (2, 1), (3, 1)]
    # under its own plant nothing leaves: no cell at step 0, nothing to pull back
    polys, Phi, phi, succ = xc.one_d_loop(2)
    assert xref.exit_reference(polys, Phi, phi, succ, 1e-8)[0] == []
    assert iref.backward_reference(polys, Phi, phi, ic.predecessors_of(succ), [], 1e-8) == ([], [], True)


def test_reference_on_the_rotation_grid():
    """step 1 is empty (invariant_cases.rotation_grid): every cell x 16 candidate predecessors, none with a radius above tol"""
    polys, Phi, phi, succ = ic.rotation_grid()
    pieces, knife = xref.exit_reference(polys, Phi, phi, succ, 1e-8)
    assert sorted(set(p[0] for p in pieces)) == [0, 3, 12, 15]           # a triangle may come in two pieces, split along a grid line's preimage
    cells, items, conv = iref.backward_reference(polys, Phi, phi, ic.predecessors_of(succ), [(s, r) for s, r, _, _ in pieces], 1e-8)
    assert conv and len(cells) == len(pieces) and len(items) == 16 * len(pieces) and all(i['outcome'] == 'none' for i in items)


def test_ordering_of_items_and_cells():
    """two regions that precede each other and themselves: the items of a step go by parent cell, then by region ascending, whatever the
    order of the predecessor lists; the cells of a step keep item order"""
    polys = [xc.box_rows([0, 0], [1, 1]), xc.box_rows([1, 0], [2, 1])]
    Phi = numpy.tile(numpy.eye(2), (2, 1, 1))
    phi = numpy.array([[0.5, 0.0], [0.5, 0.0]])
    cells0 = [(1, xc.box_rows([1.5, 0], [2, 1]))]                        # the states of region 1 that leave through x = 2
    cells, items, conv = iref.backward_reference(polys, Phi, phi, [[1, 0], [1, 0]], cells0, 1e-8)
    assert [(i['step'], i['parent'], i['region']) for i in items][:4] == [(1, 0, 0), (1, 0, 1), (2, 1, 0), (2, 1, 1)]
    assert conv and [(c['step'], c['source'], c['parent']) for c in cells] == [(0, 1, -1), (1, 1, 0), (2, 0, 1), (3, 0, 2)]
    x_range = lambda rows: (float(numpy.max(-rows[rows[:, 1] < 0][:, 0])), float(numpy.min(rows[rows[:, 1] > 0][:, 0])))
    assert numpy.allclose([x_range(c['rows']) for c in cells], [(1.5, 2.0), (1.0, 1.5), (0.5, 1.0), (0.0, 0.5)], rtol=0, atol=1e-12)
    assert [c['lineage'] for c in cells] == [(0,), (0, 1), (0, 1, 0), (0, 1, 0, 0)]


def test_reference_knife_share_of_the_first_set():
    """two steps of the first synthetic set on the CPU: no knife item (the counts of all sets with max_steps = 4 are in DESIGN §3.23)"""
    case = ic.SETS[0]
    polys, Phi, phi = xc.synthetic_set(*case)
    succ, _ = xref.successors_reference(polys, Phi, phi, ic.TOL)
    pieces, _ = xref.exit_reference(polys, Phi, phi, succ, ic.TOL)
    cells, items, _ = iref.backward_reference(polys, Phi, phi, ic.predecessors_of(succ), [(s, r) for s, r, _, _ in pieces], ic.TOL, 2)
    assert len(items) > 100 and sum(i['knife'] for i in items) <= ic.KNIFE_CAP * len(items)
    assert [sum(c['step'] == k for c in cells) for k in range(3)] == [24, 31, 52]


def _hand_made():
    """[0, 4] in two regions [0, 2] and [2, 4]; cells: [3, 4] at step 0 (region 1), [2, 3] and [1.5, 2] at step 1, [1, 1.5] at step 2"""
    off, ef = xc.csr([xc.box_rows([0], [2]), xc.box_rows([2], [4])])
    coff, crow = xc.csr([xc.box_rows([3], [4]), xc.box_rows([2], [3]), xc.box_rows([1.5], [2]), xc.box_rows([1], [1.5])])
    return inv.InvariantSet(n_regions=2, cell_off=coff, cell_rows=crow, source=numpy.array([1, 1, 0, 0]), step=numpy.array([0, 1, 1, 2]),
                            parent=numpy.array([-1, 0, 0, 2]), wide=numpy.zeros(4, dtype=bool), converged=True, steps=2, region_off=off, region_rows=ef)


def test_exit_step_and_contains_on_hand_made_cells():
    s = _hand_made()
    th = numpy.array([[3.5], [2.5], [1.7], [1.2], [0.5], [-0.1], [4.1], [3.0], [2.0], [1.5]])
    # a point on a shared boundary belongs to the first cell that holds it: the earliest exit
    assert s.exit_step(th).tolist() == [1, 2, 2, 3, 0, -1, -1, 1, 2, 2]
    assert s.contains(th).tolist() == [False, False, False, False, True, False, False, False, False, False]
    assert s.exit_step(numpy.array([4.05]), tol=0.1).tolist() == [1] and s.exit_step(numpy.zeros((0, 1))).tolist() == []
    assert s.cells_of(0).tolist() == [2, 3] and s.cells_of(1).tolist() == [0, 1] and len(s) == 4 and len(s.polytopes()) == 4
    assert s.rows_of(3).tolist() == [[1.5, 1.0], [-1.0, -1.0]]
    with pytest.raises(ValueError, match='thetas must be'):
        s.exit_step(numpy.zeros((3, 2)))
    empty = inv.InvariantSet(n_regions=2, cell_off=numpy.zeros(1, dtype=numpy.int64), cell_rows=numpy.zeros((0, 2)), source=numpy.zeros(0, dtype=numpy.int64),
                             step=numpy.zeros(0, dtype=numpy.int64), parent=numpy.zeros(0, dtype=numpy.int64), wide=numpy.zeros(0, dtype=bool),
                             converged=True, steps=0, region_off=s.region_off, region_rows=s.region_rows)
    assert empty.exit_step(th).tolist() == [0, 0, 0, 0, 0, -1, -1, 0, 0, 0]


def test_replay_on_the_one_d_hand_case():
    polys, Phi, phi, _ = xc.one_d_loop(4)
    th = numpy.array([[0.5], [0.2], [0.1], [0.02], [0.004], [0.0], [0.8], [-0.06]])
    step, near = iref.replay_exit_step(polys, Phi, phi, th, 6)
    assert step.tolist() == [1, 1, 2, 3, 4, 0, -1, 2] and near.min() > 1e-3


def test_every_value_error_comes_before_the_library(monkeypatch):
    from ppopt_amd import _lib
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('the library was touched'))
    polys, Phi, phi, succ = xc.one_d_loop(4)
    off, ef = xc.csr(polys)
    coff, crow = xc.csr([r for _, r in ic.one_d_cells0()])
    base = dict(row_off=off, ef_rows=ef, Phi=Phi, phi=phi, n_t=1, predecessors=ic.predecessors_of(succ), cell_off=coff, cell_rows=crow,
                cell_source=[0, 1, 1, 2], tol=1e-8, max_steps=4, max_cells=64)
    big = numpy.tile(xc.box_rows([0], [1]), (129, 1))
    for kw, text in (({'n_t': 0}, 'outside 1..16'), ({'n_t': 17}, 'outside 1..16'), ({'tol': -1.0}, 'tol'), ({'tol': numpy.nan}, 'tol'),
                     ({'max_steps': -1}, 'max_steps'), ({'max_cells': 0}, 'max_cells'), ({'max_rows_total': 0}, 'max_rows_total'),
                     ({'row_off': off[1:]}, 'must describe'), ({'Phi': Phi[:2]}, 'must describe'), ({'phi': phi[:, :0]}, 'must describe'),
                     ({'row_off': [0, 0, 4, 6]}, '1..256 rows'), ({'row_off': [0, 258], 'ef_rows': big, 'Phi': Phi[:1], 'phi': phi[:1]}, '1..256 rows'),
                     ({'ef_rows': ef * numpy.inf}, 'finite'), ({'Phi': Phi * numpy.nan}, 'finite'), ({'predecessors': [[1]]}, 'one index list'),
                     ({'predecessors': [[3], [], []]}, 'must name polytopes'), ({'predecessors': [[-1], [], []]}, 'must name polytopes'),
                     ({'cell_off': coff[:-1]}, 'cell_off'), ({'cell_source': [0, 1, 1]}, 'cell_off'), ({'cell_off': [0, 0, 4, 6, 8]}, 'every cell needs'),
                     ({'cell_off': [0, 258], 'cell_rows': big, 'cell_source': [0], 'max_rows_total': 1000}, 'every cell needs'),
                     ({'cell_source': [0, 1, 1, 3]}, 'cell_source'), ({'cell_source': [0, -1, 1, 2]}, 'cell_source'),
                     ({'cell_rows': crow * numpy.nan}, 'cell rows must be finite'), ({'max_cells': 3}, 'step 0'), ({'max_rows_total': 7}, 'step 0')):
        with pytest.raises(ValueError, match=text):
            inv.backward_exit_cells(**dict(base, **kw))
    # max_steps = 0 and an empty step 0 need no library either
    got = inv.backward_exit_cells(**dict(base, max_steps=0))
    assert len(got) == 4 and got.status == 'MAX_STEPS' and not got.converged and got.steps == 0 and got.exit_step(numpy.array([[0.2], [0.1]])).tolist() == [1, 0]
    none = inv.backward_exit_cells(**dict(base, cell_off=[0], cell_rows=numpy.zeros((0, 2)), cell_source=[]))
    assert len(none) == 0 and none.converged and none.status == 'CONVERGED'
