"""Search trees on the device: mpc_tree_build against the independent CPU reference and its exact checker (check_tree:
no region leaves a subtree that its points reach) on the cases and builder arguments of search_tree_cases.py, determinism, and tree
location identical to the scan (and the walk where it applies) on witness points and on solved programs."""
import warnings

import numpy
import pytest

import search_tree_cases as stc
import search_tree_reference as ref
from ppopt_amd import _lib
from ppopt_amd.upop import SearchTree
from search_tree_cases import _random_polytopes
from test_search_tree_cpu import CASES, _Prog, _region, reference_tree
from ppopt_amd.solution import Solution

pytestmark = pytest.mark.gpu

KNIFE = 1e-9   # classification differences are allowed only for pairs whose reference lo / hi lies this close to -w / +w


def _knife_pairs(t, band):
    plus, minus, lo, hi, _ = t['classification']
    return int(numpy.sum(numpy.abs(lo + band) <= KNIFE) + numpy.sum(numpy.abs(hi - band) <= KNIFE))


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_tree_equals_the_reference(name):
    sol = CASES[name]
    t = reference_tree(sol)
    dev = sol.search_tree()
    assert dev.stats['pairs'] == len(sol.critical_regions) * len(dev.planes)
    assert numpy.array_equal(dev.planes, t['planes'])
    assert _knife_pairs(t, 16 * sol.point_location_tolerance) == 0
    for k in ('node_plane', 'node_child', 'node_off', 'items'):
        assert numpy.array_equal(getattr(dev, k), t[k]), k
    assert numpy.all(dev.node_tau >= t['tau_raw'] - 1e-12)
    # the allowance grows with |o| and |theta*|_1: bounded by twice the reference's widened tau
    assert numpy.all(dev.node_tau <= 2.0 * t['node_tau'] + 1e-12)


@pytest.mark.parametrize('n,m,R', [(3, 8, 12), (6, 24, 10), (16, 40, 6), (4, 256, 3)])
def test_random_polytopes_against_the_reference(n, m, R):
    rng = numpy.random.default_rng(n * 100 + m)
    sol = Solution(_Prog(2, n, rng), _random_polytopes(rng, n, m, R), point_location_tolerance=1e-5)
    t = reference_tree(sol)
    dev = sol.search_tree()
    assert _knife_pairs(t, 16e-5) == 0
    for k in ('node_plane', 'node_child', 'node_off', 'items'):
        assert numpy.array_equal(getattr(dev, k), t[k]), k
    assert numpy.all(dev.node_tau >= t['tau_raw'] - 1e-12)
    pts = numpy.vstack([rng.normal(size=(20000, n)) * 5.0] + [numpy.linalg.lstsq(cr.E, cr.f.ravel() - 0.05, rcond=None)[0] + rng.normal(size=(200, n)) * 1e-3
                                                               for cr in sol.critical_regions])
    for inclusive in (False, True):
        assert numpy.array_equal(dev.locate_batch(pts, inclusive=inclusive), sol.get_region_batch(pts, inclusive=inclusive))


def test_two_builds_are_identical():
    sol = CASES['tiny_far']
    a = SearchTree.build(sol)
    b = SearchTree.build(sol)
    for k in ('planes', 'node_plane', 'node_child', 'node_tau', 'node_off', 'items'):
        assert numpy.array_equal(getattr(a, k), getattr(b, k))


# ---- soundness of device-built trees by the exact checker (search_tree_reference.check_tree, search_tree_cases.py) -----------------------
_ARRAYS = ('planes', 'node_plane', 'node_child', 'node_tau', 'node_off', 'items')


def _device_tree(name, leaf_size=1, max_depth=48, band=None, own=True):
    """(SearchTree, arrays, stats) of a case built through Locator.build_tree with the case's plane list"""
    c = stc.case(name)
    band = c.band if band is None else band
    cand = c.cand if own and c.cand is not None else (None, None)
    loc = c.sol.locator()
    stats = loc.build_tree(c.planes, cand[0], cand[1], c.tol, band, leaf_size, max_depth)
    arrays = loc.get_tree()
    tree = SearchTree(c.sol, arrays, c.tol, band, stats)
    loc.tree_owner = tree
    return tree, arrays, stats


def _check_device_tree(name, leaf_size=1, max_depth=48, band=None, own=True):
    c = stc.case(name)
    t = stc.reference(name, leaf_size, max_depth, band, own)
    tree, arrays, stats = _device_tree(name, leaf_size, max_depth, band, own)
    rec = stc.check(name, arrays, leaf_size, max_depth, band, own)
    print(name, leaf_size, max_depth, band, own, 'nodes', len(arrays['node_plane']), 'dropped', rec['dropped'], 'margin', rec['margin'],
          {k: v for k, v in rec.items() if isinstance(v, list) and v})
    assert rec['structure'] == []
    assert rec['unsound'] == [] and rec['missing'] == [], 'the tree loses points of a region'
    assert rec['not_one_sided'] == [] and rec['loose'] == [] and rec['stopped_early'] == []
    assert numpy.array_equal(arrays['planes'], t['planes'])
    for k in ('node_plane', 'node_child', 'node_off', 'items'):
        assert numpy.array_equal(arrays[k], t[k]), k
    assert stats['capped'] == 0
    assert stats['pairs'] == c.n_regions * len(c.planes)
    assert stats['tau_lps'] == rec['dropped']
    return tree, arrays, rec


@pytest.mark.parametrize('name', stc.NAMES)
def test_device_tree_is_sound(name):
    _, arrays, rec = _check_device_tree(name)
    assert rec['dropped'] > 0 and rec['margin'] > 0.0
    if name == 'planes_257':
        assert arrays['node_plane'].max() >= 256, 'a winner of the second chunk of k_tree_split'
    if name == 'edges':
        leaves = numpy.flatnonzero(arrays['node_plane'] < 0)
        for j in stc.EDGE_EMPTY + (stc.EDGE_NO_ROWS,):
            assert all(j in arrays['items'][arrays['node_off'][k]:arrays['node_off'][k + 1]] for k in leaves)


@pytest.mark.parametrize('leaf_size,max_depth,band,own', stc.ARGS)
@pytest.mark.parametrize('name', stc.ARG_CASES)
def test_device_tree_is_sound_for_every_builder_argument(name, leaf_size, max_depth, band, own):
    _check_device_tree(name, leaf_size, max_depth, band, own)


@pytest.mark.parametrize('name', stc.NAMES)
def test_witness_points_are_located_as_the_scan_locates_them(name):
    """the point of every dropped region farthest over its node's plane, pulled 1e-3 of the way to the region's centre: the first point a
    short tau would lose"""
    c = stc.case(name)
    dev, arrays, _ = _device_tree(name)
    pts, nodes, regions, with_dropped = stc.witnesses(name, arrays)
    assert with_dropped and set(nodes.tolist()) == set(with_dropped)
    sol, loc = c.sol, c.sol.locator()
    for inclusive in (False, True):
        want = sol.get_region_batch(pts, inclusive=inclusive)
        assert (want >= 0).any()
        assert numpy.array_equal(dev.locate_batch(pts, inclusive=inclusive), want), (name, inclusive)
        assert numpy.array_equal([dev.locate(th, inclusive=inclusive) for th in pts], want), (name, inclusive)
        half = 0.5 * c.tol
        want = loc.query(pts, half, sol.is_overlapping, want_x=False, inclusive=inclusive)[0]
        assert numpy.array_equal(loc.query(pts, half, sol.is_overlapping, want_x=False, inclusive=inclusive, tree=True)[0], want), (name, inclusive)
        assert numpy.array_equal([dev.locate(th, inclusive=inclusive, tol=half) for th in pts], want), (name, inclusive)
    if name == 'edges':   # empty regions are never located; the scan never meets the region without rows
        assert not set(sol.get_region_batch(pts).tolist()) & set(stc.EDGE_EMPTY + (stc.EDGE_NO_ROWS,))


def test_two_builds_of_a_deep_partition_are_identical_bytes():
    a = _device_tree('part_2_6')[1]
    b = _device_tree('part_2_6')[1]
    assert len(a['node_plane']) == 127
    for k in _ARRAYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def _solve(name):
    from ppopt_amd import MPLP_Program, problem_generator as pg
    from ppopt_amd.mp_solvers import mpqp_hip_combinatorial
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    import bench
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if name == 'c2x20':
            return solve_mpqp(bench.build_program('c2x20'), mpqp_algorithm.combinatorial)
        if name == 'c3_l4':
            return mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4)
        if name == 'c1_mplp':
            d = pg.transport_mplp_data()
            prog = MPLP_Program(d['A'], d['b'], d['c'], d['H'], d['A_t'], d['b_t'], d['F'], equality_indices=list(d['equality_indices']))
            return solve_mpqp(prog, mpqp_algorithm.combinatorial)
        if name == 'mi_market':
            from test_export import mixed_integer_solution
            return mixed_integer_solution('mpMIQP_market_problem')[0]
    raise KeyError(name)


def _points(sol, rng, n=100_000):
    """uniform points over the regions' bounding box and beyond, plus points at +-{0.5, 1.01} tol from facet centres"""
    ef, row_off, _ = sol._stacked()
    n_t = ef.shape[1] - 1
    centre, radius, status = _lib.facet_centres(ef, row_off)
    ok = (status == 0) & numpy.all(numpy.isfinite(centre), axis=1)
    c = centre[ok]
    lo, hi = c.min(axis=0), c.max(axis=0)
    span = numpy.maximum(hi - lo, 1e-3)
    pts = [rng.uniform(lo - 0.2 * span, hi + 0.2 * span, size=(n // 2, n_t))]
    E = ef[ok, 1:]
    nrm = numpy.linalg.norm(E, axis=1, keepdims=True)
    tol = sol.point_location_tolerance
    pick = rng.integers(0, len(c), size=n // 2)
    k = rng.choice([-1.01, -0.5, 0.5, 1.01], size=(n // 2, 1))
    pts.append(c[pick] + k * tol * E[pick] / nrm[pick] ** 2 * numpy.maximum(1.0, nrm[pick]))
    return numpy.vstack(pts)


@pytest.mark.parametrize('name', ['c2x20', 'c3_l4', 'c1_mplp', 'mi_market'])
def test_tree_location_is_the_scan(name):
    sol = _solve(name)
    tree = sol.search_tree()
    assert sol.search_tree() is tree
    pts = _points(sol, numpy.random.default_rng(7))
    assert len(pts) >= 100_000
    for inclusive in (False, True):
        want = sol.get_region_batch(pts, inclusive=inclusive)
        got = tree.locate_batch(pts, inclusive=inclusive)
        assert numpy.array_equal(got, want), (name, inclusive, int(numpy.sum(got != want)))
        assert (want >= 0).any() and (want < 0).any()
    x_s, r_s = sol.evaluate_batch(pts)
    x_t, r_t = tree.evaluate_batch(pts)
    assert numpy.array_equal(r_s, r_t) and numpy.array_equal(x_s, x_t, equal_nan=True)
    loc = sol.locator()
    half = 0.5 * sol.point_location_tolerance
    for inclusive in (False, True):
        scan = loc.query(pts, half, sol.is_overlapping, want_x=False, inclusive=inclusive)[0]
        assert numpy.array_equal(loc.query(pts, half, sol.is_overlapping, want_x=False, inclusive=inclusive, tree=True)[0], scan)
    if not sol.is_overlapping:
        walk = loc.query(pts, sol.point_location_tolerance, False, want_x=False, walk=True)[0]
        assert numpy.array_equal(walk, sol.get_region_batch(pts))


def test_refusals():
    rng = numpy.random.default_rng(1)
    sol = CASES['triangles']
    loc = sol.locator()
    ef, row_off, xlaw = sol._stacked()
    fresh = _lib.Locator(row_off, ef, xlaw)
    with pytest.raises(_lib.MpcError, match='without an attached tree'):
        fresh.query(numpy.zeros((4, 2)), 1e-5, tree=True)
    fresh.close()
    tree = sol.search_tree()
    tree.locate_batch(numpy.zeros((3, 2)))
    with pytest.raises(_lib.MpcError, match='larger than the tolerance'):
        loc.query(numpy.zeros((4, 2)), 2e-5, tree=True)
    planes = tree.planes
    with pytest.raises(_lib.MpcError, match='budget'):
        loc.build_tree(planes, None, None, 1e-5, 1.6e-4, budget=8)
    big = Solution(_Prog(2, 17, rng), [_region(numpy.eye(17), numpy.ones(17), rng)], point_location_tolerance=1e-5)
    with pytest.raises(_lib.MpcError):
        SearchTree.build(big)
