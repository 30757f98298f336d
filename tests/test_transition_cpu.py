"""The host side of Solution.transition_graph without a device: the CPU reference on hand-computed cases, the box sweep
against the brute-force test of all pairs, the graph queries on hand-made graphs and the refusals that come before any launch."""
import numpy
import pytest

import transition_reference as ref
from ppopt_amd import _lib, transition as tr
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.solution import Solution
from ppopt_amd.transition import TransitionGraph, image_box_pairs

TOL = 1e-8


def box_rows(lo, hi):
    """unit rows [o | n] of the box lo <= theta <= hi"""
    lo, hi = numpy.asarray(lo, dtype=float), numpy.asarray(hi, dtype=float)
    n = len(lo)
    return numpy.vstack([numpy.column_stack([hi, numpy.eye(n)]), numpy.column_stack([-lo, -numpy.eye(n)])])


# ---- the reference on cases worked out by hand ----------------------------------------------------------------------------------------
def test_reference_one_d_loop():
    """min u^2, |u| <= 1, |2 theta + u| <= 0.5: M = [-1/4, 1/4] with u = 0 (theta+ = 2 theta), U = [1/4, 3/4] with theta+ = 1/2 and
    L = [-3/4, -1/4] with theta+ = -1/2.  T_MM = [-1/8, 1/8], T_MU = [1/8, 1/4], T_ML = [-1/4, -1/8]; U and L map to one point each,
    inside themselves: T_UU = U, T_LL = L, and every row of the other targets is constant with beta = -1/4 or less."""
    polys = [box_rows([-0.25], [0.25]), box_rows([0.25], [0.75]), box_rows([-0.75], [-0.25])]
    Phi = numpy.array([[[2.0]], [[0.0]], [[0.0]]])
    phi = numpy.array([[0.0], [0.5], [-0.5]])
    got = ref.graph_reference(polys, Phi, phi, TOL)
    want = {(0, 0): 0.125, (0, 1): 0.0625, (0, 2): 0.0625, (1, 1): 0.25, (2, 2): 0.25}
    for pair, (status, r, knife) in got.items():
        assert not knife, pair
        if pair in want:
            assert status == ref.EDGE and abs(r - want[pair]) <= 1e-12, (pair, status, r)
        else:
            assert status == ref.NO_EDGE and r == -numpy.inf, (pair, status, r)


def test_reference_rotation_is_a_four_cycle():
    """the square [-1, 1]^2 in quadrants, counter-clockwise from [0, 1]^2, all turned by 90 degrees: quadrant k goes onto quadrant k + 1
    (radius 1/2); the image meets every other quadrant in a facet or a vertex, radius 0, which is no edge"""
    quads = [box_rows([0, 0], [1, 1]), box_rows([-1, 0], [0, 1]), box_rows([-1, -1], [0, 0]), box_rows([0, -1], [1, 0])]
    Phi = numpy.tile(numpy.array([[0.0, -1.0], [1.0, 0.0]]), (4, 1, 1))
    got = ref.graph_reference(quads, Phi, numpy.zeros((4, 2)), TOL)
    for (i, j), (status, r, knife) in got.items():
        if j == (i + 1) % 4:
            assert status == ref.EDGE and abs(r - 0.5) <= 1e-12 and not knife
        else:
            assert status == ref.NO_EDGE and abs(r) <= 1e-12 and knife       # r = 0 lies within KNIFE of tol
    edges = [pair for pair, v in got.items() if v[0] != ref.NO_EDGE]
    g = TransitionGraph.from_edges(4, [e[0] for e in edges], [e[1] for e in edges])
    assert [c.tolist() for c in g.cycles_outside([])] == [[0, 1, 2, 3]]
    assert g.reachable([2]).tolist() == [0, 1, 2, 3]


def test_reference_nilpotent_map():
    """(x, y) -> (y, 1/2) on the upper half U = [-1, 1] x [0, 1] and the lower half L = [-1, 1] x [-1, 0] of the square: Phi^2 = 0.  The rows
    of a target in y are constant: y+ = 1/2 satisfies U's (dropped) and breaks L's row y <= 0 (beta = -1/2); the rows in x become
    |y| <= 1.  So T_UU = U and T_LU = L (radius 1/2), T_UL and T_LL are empty."""
    polys = [box_rows([-1, 0], [1, 1]), box_rows([-1, -1], [1, 0])]
    Phi = numpy.tile(numpy.array([[0.0, 1.0], [0.0, 0.0]]), (2, 1, 1))
    phi = numpy.tile(numpy.array([0.0, 0.5]), (2, 1))
    got = ref.graph_reference(polys, Phi, phi, TOL)
    assert got[(0, 0)][:2] == (ref.EDGE, 0.5) and got[(1, 0)][:2] == (ref.EDGE, 0.5)
    assert got[(0, 1)][:2] == (ref.NO_EDGE, -numpy.inf) and got[(1, 1)][:2] == (ref.NO_EDGE, -numpy.inf)
    assert not any(v[2] for v in got.values())
    back, empty, knife = ref.pulled_back(polys[0], Phi[0], phi[0], TOL)
    assert len(back) == 2 and not empty and not knife
    numpy.testing.assert_allclose(back, [[1.0, 0.0, 1.0], [1.0, 0.0, -1.0]])


def test_reference_unbounded_and_row_threshold():
    cone = numpy.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [-numpy.sqrt(0.5), -numpy.sqrt(0.5), -numpy.sqrt(0.5)]])     # x, y >= 0, x + y >= 1
    status, r, knife = ref.pair_reference(cone, cone, numpy.eye(2), numpy.zeros(2), TOL)
    assert status == ref.UNBOUNDED and r == numpy.inf and not knife
    sq = box_rows([0, 0], [1, 1])
    assert ref.pair_reference(sq, sq, 1e-12 * numpy.eye(2), numpy.array([0.5, 0.5]), TOL)[2]          # |a| = the threshold itself
    assert not ref.pair_reference(sq, sq, 1e-14 * numpy.eye(2), numpy.array([0.5, 0.5]), TOL)[2]
    assert ref.pair_reference(sq, sq, 1e-14 * numpy.eye(2), numpy.array([0.5, 0.5]), TOL)[:2] == (ref.EDGE, 0.5)
    assert ref.pair_reference(sq, sq, numpy.eye(2), numpy.array([1.0 - 2e-8, 0.0]), TOL)[2]           # radius 1e-8: at tol


# ---- the sweep -----------------------------------------------------------------------------------------------------------------------
def _brute(image_box, region_box, usable, tol):
    out = []
    for i in numpy.flatnonzero(usable):
        for j in numpy.flatnonzero(usable):
            sep = False
            for t in range(image_box.shape[2]):
                four = (image_box[i, 0, t], image_box[i, 1, t], region_box[j, 0, t], region_box[j, 1, t])
                if not any(numpy.isnan(v) for v in four):      # a NaN bound separates nothing
                    sep = sep or min(four[1], four[3]) - max(four[0], four[2]) <= -tol
            if not sep:
                out.append((int(i), int(j)))
    return sorted(out)


@pytest.mark.parametrize('n,seed,k', [(1, 0, 30), (2, 1, 60), (3, 2, 80), (5, 3, 50)])
def test_image_box_pairs_against_all_pairs(n, seed, k):
    rng = numpy.random.default_rng(seed)

    def boxes():
        c, s = rng.uniform(-1, 1, (k, n)), rng.uniform(0.02, 0.6, (k, n))
        return numpy.stack([c - s, c + s], axis=1)

    image, region = boxes(), boxes()
    image[rng.random(k) < 0.1, 0, 0] = -numpy.inf            # infinite along the sweep coordinate
    image[rng.random(k) < 0.1, 1, 0] = numpy.inf
    image[rng.random(k) < 0.1, 1, n - 1] = numpy.inf
    image[3] = numpy.array([[-numpy.inf] * n, [numpy.inf] * n])
    region[rng.random(k) < 0.1, 0, n - 1] = -numpy.inf
    region[5, 1, 0] = numpy.inf
    image[7, 0, 0] = numpy.nan                                # a NaN bound must not drop a pair
    image[8, 1, n - 1] = numpy.nan
    # boxes that touch exactly: the gap 0 > -tol keeps them
    image[12] = numpy.array([[0.1] * n, [0.3] * n])
    region[11, 0] = image[12, 1]
    region[11, 1] = image[12, 1] + 0.1
    usable = rng.random(k) > 0.1
    usable[[3, 5, 7, 8, 11, 12]] = True
    for tol in (1e-8, 0.0, 0.05):
        pa, pb = image_box_pairs(image, region, usable, tol)
        assert list(zip(pa.tolist(), pb.tolist())) == _brute(image, region, usable, tol)
    assert (12, 11) in set(zip(*[a.tolist() for a in image_box_pairs(image, region, usable, 1e-8)]))
    pa, pb = image_box_pairs(image, region, numpy.zeros(k, dtype=bool), 1e-8)
    assert len(pa) == 0 and len(pb) == 0


# ---- the graph queries -----------------------------------------------------------------------------------------------------------------
def _graph(n, edges):
    return TransitionGraph.from_edges(n, [e[0] for e in edges], [e[1] for e in edges])


def _same_as_enumeration(n, edges, target):
    lower, upper = _graph(n, edges).steps_to(target)
    lo, up = ref.steps_to_reference(n, edges, target)
    numpy.testing.assert_array_equal(lower, lo)
    numpy.testing.assert_array_equal(upper, up)
    return lower.tolist(), upper.tolist()


def test_steps_to_chain():
    edges = [(3, 2), (2, 1), (1, 0), (0, 0)]
    assert _same_as_enumeration(4, edges, [0]) == ([0, 1, 2, 3], [0, 1, 2, 3])
    g = _graph(4, edges)
    assert g.successors(2).tolist() == [1] and g.predecessors(0).tolist() == [0, 1] and g.predecessors(3).tolist() == []
    assert g.reachable([2]).tolist() == [0, 1, 2] and g.reachable([]).tolist() == []
    assert g.cycles_outside([0]) == [] and [c.tolist() for c in g.cycles_outside([])] == [[0]]
    assert g.has_edge(0, 0) and not g.has_edge(0, 1)


def test_steps_to_diamond_with_unequal_paths():
    # 4 -> 1 -> 0 and 4 -> 3 -> 2 -> 1 -> 0
    edges = [(4, 1), (4, 3), (3, 2), (2, 1), (1, 0), (0, 0)]
    assert _same_as_enumeration(5, edges, [0]) == ([0, 1, 2, 3, 2], [0, 1, 2, 3, 4])
    assert _graph(5, edges).indices.tolist() == [0, 0, 1, 2, 1, 3]


def test_steps_to_self_loop_outside_the_target():
    inf = numpy.inf
    edges = [(3, 2), (2, 2), (2, 1), (1, 0), (0, 0), (4, 1)]
    assert _same_as_enumeration(5, edges, [0]) == ([0, 1, 2, 3, 2], [0, 1, inf, inf, 2])
    g = _graph(5, edges)
    assert [c.tolist() for c in g.cycles_outside([0])] == [[2]]
    # a cycle of two regions, and one that only reaches it
    edges = [(1, 2), (2, 1), (2, 0), (3, 1), (0, 0)]
    assert _same_as_enumeration(4, edges, [0]) == ([0, 2, 1, 3], [0, inf, inf, inf])
    assert [c.tolist() for c in _graph(4, edges).cycles_outside([0])] == [[1, 2]]


def test_steps_to_dead_end():
    inf = numpy.inf
    # 3 has no successor; 2 may go there or to the target; 4 reaches nothing but the dead end
    edges = [(2, 3), (2, 0), (1, 0), (4, 3), (0, 0)]
    assert _same_as_enumeration(5, edges, [0]) == ([0, 1, 1, inf, inf], [0, 1, inf, inf, inf])


def test_steps_to_refuses_a_target_that_is_not_closed():
    g = _graph(3, [(0, 0), (0, 1), (1, 2), (2, 0)])
    with pytest.raises(ValueError, match=r'0 -> 1 leaves it'):
        g.steps_to([0])
    lower, upper = g.steps_to([0, 1, 2])
    assert lower.tolist() == upper.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match='regions must lie in'):
        g.steps_to([3])


@pytest.mark.parametrize('seed', range(6))
def test_steps_to_random_graphs_against_enumeration(seed):
    rng = numpy.random.default_rng(seed)
    n = 8
    edges = sorted({(int(i), int(j)) for i, j in rng.integers(0, n, size=(14, 2)) if i != 0} | {(0, 0)})
    _same_as_enumeration(n, edges, [0])


def test_from_edges_sorts_and_carries_the_edge_data():
    g = TransitionGraph.from_edges(3, [2, 0, 2], [1, 2, 0], radius=[0.3, 0.1, 0.2], status=[tr.EDGE, tr.UNBOUNDED, tr.UNDECIDED],
                                   witness=[[3.0], [1.0], [2.0]])
    assert g.indptr.tolist() == [0, 1, 1, 3] and g.indices.tolist() == [2, 0, 1]
    assert g.radius.tolist() == [0.1, 0.2, 0.3] and g.status.tolist() == [tr.UNBOUNDED, tr.UNDECIDED, tr.EDGE] and g.witness[:, 0].tolist() == [1.0, 2.0, 3.0]
    assert g.sources().tolist() == [0, 2, 2]
    with pytest.raises(ValueError):
        TransitionGraph.from_edges(2, [0], [2])
    assert tr.STATUS == ('NO_EDGE', 'EDGE', 'UNBOUNDED', 'UNDECIDED')
    assert (_lib.TRANSITION_NO_EDGE, _lib.TRANSITION_EDGE, _lib.TRANSITION_UNBOUNDED, _lib.TRANSITION_UNDECIDED) == (0, 1, 2, 3)


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


def test_transition_graph_refusals(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the device was touched')
    for name in ('merge_regions', 'transition_boxes', 'transition_pairs', 'load'):
        monkeypatch.setattr(_lib, name, boom)
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
                                (_stub(rows=260), (A, B, [0]), {}, 'more than 256 rows')):
        with pytest.raises(ValueError, match='transition_graph: .*' + text):
            sol.transition_graph(*args, **kw)
    wide = _stub(n_t=17)
    with pytest.raises(ValueError, match='n_theta = 17 > 16'):
        wide.transition_graph(numpy.eye(17), numpy.ones((17, 1)), [0])


def test_the_shared_check_still_speaks_for_the_certificate():
    """invariance._check with its default name: the messages certify_recursive_feasibility always gave"""
    from ppopt_amd import invariance
    with pytest.raises(ValueError, match=r'certify_recursive_feasibility: A must be \[2, 2\]'):
        invariance._check(_stub(), numpy.eye(3), numpy.ones((2, 1)), [0], None, None, 1e-7)
    with pytest.raises(ValueError, match='certify_recursive_feasibility: B must be finite'):
        invariance._check(_stub(), numpy.eye(2), numpy.full((2, 1), numpy.inf), [0], None, None, 1e-7)


def test_transition_pairs_refuses_bad_arrays_on_the_host(monkeypatch):
    monkeypatch.setattr(_lib, 'merge_regions', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the device was touched')))
    sq = box_rows([0, 0], [1, 1])
    off, ef = numpy.array([0, 4, 8]), numpy.vstack([sq, sq])
    Phi, phi = numpy.tile(numpy.eye(2), (2, 1, 1)), numpy.zeros((2, 2))
    for kw, text in (({'tol': -1.0}, 'tol'), ({'Phi': Phi[:1]}, 'must describe'), ({'phi': phi * numpy.nan}, 'finite'), ({'n_t': 17}, 'outside 1..16'),
                     ({'off': numpy.array([0, 0, 8])}, '1..256 rows')):
        a = dict(off=off, ef=ef, Phi=Phi, phi=phi, n_t=2, tol=TOL)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            if a['n_t'] == 17:
                tr.transition_pairs(numpy.array([0, 4]), numpy.hstack([numpy.ones((4, 1)), numpy.eye(17)[:4]]), numpy.eye(17)[None], numpy.zeros((1, 17)), 17)
            else:
                tr.transition_pairs(a['off'], a['ef'], a['Phi'], a['phi'], a['n_t'], tol=a['tol'])
