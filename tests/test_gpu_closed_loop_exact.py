"""k_simulate against the exact host reference (closed_loop_reference.simulate_rows), at the C-ABI level: synthetic partitions with
lattice laws and plants (tests/closed_loop_cases.py), no program is solved.  Every case is certified exact on the host
(tests/test_closed_loop_cpu.py), so the device has one admissible answer whatever its order of operations, and every comparison is an
equality of bit patterns: theta and u (a NaN is a NaN), region, status, exit_step and the step count.

Instantiations k_simulate<theta width, input width, locator> and the case that reaches each (every case runs scan, tree, walk2, walk4):
  <4, 4, *>    test_widths[*-w1u1], [*-w4u4]        <4, 16, *>   test_widths[*-w1u5], [*-w4u16]
  <8, 4, *>    test_widths[*-w5u4], [*-w8u1]        <8, 16, *>   test_widths[*-w5u5], [*-w8u16]
  <16, 4, *>   test_widths[*-w9u4], [*-w16u1]       <16, 16, *>  test_widths[*-w9u5], [*-w16u16]"""
import numpy
import pytest

import closed_loop_cases as cases
import closed_loop_reference as ref
import locate_reference as lref
from ppopt_amd import _lib, closed_loop

pytestmark = pytest.mark.gpu

MODES = ['scan', 'tree', 'walk2', 'walk4']
MODE_FLAG = {'scan': 0, 'tree': _lib.MPC_LOCATE_TREE, 'walk2': _lib.MPC_LOCATE_WALK, 'walk4': _lib.MPC_LOCATE_WALK}
_NAN = numpy.uint64(0x7ff8000000000000)


def _bits(a):
    """bit patterns, with one pattern for every NaN (the record's unwritten tail and a computed NaN are both 'not a number')"""
    a = numpy.ascontiguousarray(a, dtype=numpy.float64)
    return numpy.where(numpy.isnan(a), _NAN, a.view(numpy.uint64))


def _open(k, mode):
    """a locator of the case with what the mode needs attached"""
    loc = _lib.Locator(k['row_off'], k['ef'], k['xlaw'], k['Q'], k['cvec'], k['H'])
    try:
        if mode == 'tree':
            planes, cand_off, cand_plane = cases.planes_of(k['row_off'], k['ef'])
            loc.build_tree(planes, cand_off, cand_plane, k['tol'], k['band'])
        elif mode != 'scan':
            masks, row_info, n_c = k[mode]
            assert masks.shape[1] == (2 if mode == 'walk2' else 4)
            assert loc.set_adjacency(masks, row_info, n_c)
    except BaseException:
        loc.close()
        raise
    return loc


def _run(loc, k, mode, n=None, **over):
    n = k['n'] if n is None else n
    kw = dict(c=k['c'], w=None if k['w'] is None else k['w'][:n].transpose(1, 0, 2), tol=k['tol'], stop_tol=k['stop_tol'],
              walk=mode.startswith('walk'), tree=mode == 'tree', **k['flags'])
    kw.update(over)
    return loc.simulate(k['theta0'][:n], k['steps'], k['A'], k['B'], k['inputs'], **kw)


def _same(got, want, n, steps, mode):
    """the device's record of the first n trajectories == the reference's, field by field"""
    theta, u, region, status, exit_step, stats = got
    assert numpy.array_equal(status, want['status'][:n]), numpy.flatnonzero(status != want['status'][:n])[:8]
    assert numpy.array_equal(exit_step, want['exit_step'][:n])
    bad = numpy.argwhere(region.T != want['region'][:n])
    assert bad.size == 0, (len(bad), bad[:4], [(region[s, p], want['region'][p, s]) for p, s in bad[:4]])
    assert numpy.array_equal(_bits(u.transpose(1, 0, 2)), _bits(want['u'][:n]))
    assert numpy.array_equal(_bits(theta.transpose(1, 0, 2)), _bits(want['theta'][:n]))
    assert stats['traj_steps'] == ref.count_steps(want['status'][:n], want['exit_step'][:n], steps)
    assert stats['mode'] == MODE_FLAG[mode]


def _check(name, mode, n=None):
    k, want = cases.case(name), cases.expected(name)
    n = k['n'] if n is None else n
    loc = _open(k, mode)
    try:
        got = _run(loc, k, mode, n)
    finally:
        loc.close()
    _same(got, want, n, k['steps'], mode)
    return got[5]


# ---- every width with every locator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cases.WIDTH_CASES)
@pytest.mark.parametrize('mode', MODES)
def test_widths(mode, name):
    """n_theta at both edges of the widths 4 / 8 / 16, each with an input count on either side of the input widths 4 / 16; inputs
    unsorted with a repeat, n_x = 17 / 20, c and w on and off, a stop tolerance in three of the cases"""
    stats = _check(name, mode)
    assert stats['traj_steps'] == cases.expected(name)['traj_steps']
    if mode.startswith('walk'):
        assert stats['crossings'] > 0


@pytest.mark.parametrize('n', cases.COUNTS)
@pytest.mark.parametrize('mode', MODES)
def test_trajectory_counts(mode, n):
    """partial wavefronts and workgroups: the trajectories are independent, so the first n of the case's 513 have the same record"""
    _check('counts', mode, n)


# ---- the record --------------------------------------------------------------------------------------------------------------------
def test_final_only_is_the_last_state_of_the_full_record():
    k, want = cases.case('w16u16'), cases.expected('w16u16')
    loc = _open(k, 'scan')
    try:
        full = _run(loc, k, 'scan')
        last = _run(loc, k, 'scan', final_only=True)
    finally:
        loc.close()
    _same(full, want, k['n'], k['steps'], 'scan')
    theta, u, region, status, exit_step, stats = last
    assert u is None and region is None and theta.shape == (k['n'], 16)
    assert numpy.array_equal(status, full[3]) and numpy.array_equal(exit_step, full[4]) and stats['traj_steps'] == full[5]['traj_steps']
    p = numpy.arange(k['n'])
    assert numpy.array_equal(_bits(theta), _bits(full[0][exit_step, p]))
    assert numpy.array_equal(_bits(theta), _bits(want['theta'][p, want['exit_step']])) and not numpy.isnan(theta).any()


# ---- non-finite states -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['scan', 'tree', 'walk2'])
def test_a_non_finite_state_ends_the_trajectory_with_status_3(mode):
    """one region {-theta_0 <= 1} with a zero law and A = 2^600 [[1, 0], [-1, 1]].  From (1, 1): (2^600, 0), then (inf, -inf): status 3
    at step 2.  From (1, 2): (2^600, 2^600), then (inf, -inf + inf = NaN): status 3 at step 2 as well.  The walk sees the row as one of
    the parameter set (kind 2)."""
    big = 2.0 ** 600
    row_off, ef = lref.stack([numpy.array([[1.0, -1.0, 0.0]])], 2)
    loc = _lib.Locator(row_off, ef, numpy.zeros((1, 1, 3)))
    try:
        if mode == 'tree':
            loc.build_tree(numpy.array([[1.0, 0.0, -1.0]]), None, None, lref.TOL, 16.0 * lref.TOL)
        elif mode == 'walk2':
            assert loc.set_adjacency(numpy.zeros((1, 2), dtype=numpy.uint64), numpy.array([lref.KIND_OMEGA << 16], dtype=numpy.int32), 128)
        theta, u, region, status, exit_step, stats = loc.simulate([[1.0, 1.0], [1.0, 2.0]], 4, big * numpy.array([[1.0, 0.0], [-1.0, 1.0]]), [[0.0], [0.0]],
                                                                  [0], tol=lref.TOL, walk=mode == 'walk2', tree=mode == 'tree')
    finally:
        loc.close()
    inf, nan = numpy.inf, numpy.nan
    want = numpy.array([[[1.0, 1.0], [big, 0.0], [inf, -inf], [nan, nan], [nan, nan]], [[1.0, 2.0], [big, big], [inf, nan], [nan, nan], [nan, nan]]])
    assert numpy.array_equal(_bits(theta.transpose(1, 0, 2)), _bits(want))
    assert status.tolist() == [3, 3] and exit_step.tolist() == [2, 2]
    assert region.T.tolist() == [[0, 0, -1, -1]] * 2
    assert numpy.array_equal(_bits(u[:, :, 0].T), _bits(numpy.array([[0.0, 0.0, nan, nan]] * 2)))
    assert stats['traj_steps'] == 4 and stats['mode'] == MODE_FLAG[mode]     # the visit that finds the state non-finite is no step


# ---- the order of the step, on data that round ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cases.WIDTH_CASES)
def test_step_order_on_rounding_data(name):
    """The lattice cases have one answer in any order, so they cannot see the order of the sum.  The contract fixes it (c, the A
    terms, the B terms, w; one rounded product and one rounded sum each), so with random float64 plants every theta_{k+1} of the record
    has to be the numpy replay, in that order, of the theta_k and u_k next to it -- as bits."""
    k = cases.case(name)
    rng = numpy.random.default_rng(k['n_t'] * 100 + k['n_u'])
    n, steps, n_t, n_u = 300, 3, k['n_t'], k['n_u']
    A, B = 0.5 * rng.normal(size=(n_t, n_t)) / numpy.sqrt(n_t), 0.2 * rng.normal(size=(n_t, n_u))
    c = None if k['c'] is None else 0.1 * rng.normal(size=n_t)
    w = None if k['w'] is None else 0.1 * rng.normal(size=(steps, n, n_t))
    theta0 = rng.uniform(-2.5, 2.5, size=(n, n_t))
    loc = _open(k, 'scan')
    try:
        theta, u, region, status, exit_step, stats = loc.simulate(theta0, steps, A, B, k['inputs'], c=c, w=w, tol=k['tol'])
    finally:
        loc.close()
    stepped = 0
    for s in range(steps):
        on = region[s] >= 0
        want = ref.step_in_order(theta[s][on], u[s][on], A, B, c, None if w is None else w[s][on])
        assert numpy.array_equal(want.view(numpy.uint64), numpy.ascontiguousarray(theta[s + 1][on]).view(numpy.uint64)), s
        assert numpy.isnan(theta[s + 1][~on]).all()
        stepped += int(on.sum())
    assert stepped >= n // 2


# ---- the box disturbance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['w5u4', 'w9u5', 'w16u16'])
def test_box_disturbance_is_the_array_of_its_draws(name):
    """n_theta = 5 and 9 are odd: the last coordinate takes the first half of a fresh draw.  closed_loop.disturbance_box is pinned to
    an independent Philox by tests/test_closed_loop_cpu.py; the array path is pinned by the lattice cases."""
    k = cases.case(name)
    rng = numpy.random.default_rng(k['n_t'])
    lo = rng.uniform(-0.3, 0.0, size=k['n_t'])
    hi = lo + rng.uniform(0.0, 0.5, size=k['n_t'])
    seed = (77 << 32) + 1234 + k['n_t']
    w = closed_loop.disturbance_box(seed, k['n'], k['steps'], lo, hi).transpose(1, 0, 2)
    loc = _open(k, 'scan')
    try:
        boxed = _run(loc, k, 'scan', w=None, box=(lo, hi), seed=seed)
        listed = _run(loc, k, 'scan', w=w)
        other = _run(loc, k, 'scan', w=None, box=(lo, hi), seed=seed + 1)
    finally:
        loc.close()
    for a, b in zip(boxed[:5], listed[:5]):
        assert numpy.array_equal(_bits(a), _bits(b)) if a.dtype == numpy.float64 else numpy.array_equal(a, b)
    assert boxed[5]['traj_steps'] == listed[5]['traj_steps'] > k['n']
    assert not numpy.array_equal(_bits(boxed[0][1]), _bits(other[0][1]))     # the seed matters


# ---- the rules ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cases.RULES_CASES)
@pytest.mark.parametrize('mode', ['scan', 'tree'])
def test_rules(mode, name):
    """overlapping boxes with oblique rows and a region without rows: the lowest objective (ties to the later region) and the
    inclusive row test inside a simulation, with starts exactly tol beyond a row"""
    _check(name, mode)


# ---- fallbacks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_holes_and_rows_of_unknown_kind(mode):
    """cells missing from the list and cells whose rows are of kind 3: the walk cannot cross them and hands the point to the lane's own
    list scan"""
    stats = _check('holes', mode)
    if mode.startswith('walk'):
        assert stats['fallbacks'] > 0 and stats['crossings'] > 0


@pytest.mark.parametrize('name', ['w4u4', 'rules4_overlapping'])
def test_tree_stack_overflow_goes_to_the_list_scan(name):
    """The trees of these cases are at most six levels deep (the rules case: one leaf), so no widening of tau can fill the stack of
    eight.  Nine nodes are put in front of the built tree instead: each tests plane 0 with tau- = inf (the descent always goes on to
    the next node, the old root at the end) and tau+ = 0 (a point with s <= 0 also pushes an empty leaf).  A point with s <= 0
    overflows at the ninth push and is settled by loc_scan_lane -- with `overlapping` by its objective branch --, every other point
    descends the old tree with an empty stack; the tree stays correct for both."""
    k, want = cases.case(name), cases.expected(name)
    loc = _open(k, 'tree')
    try:
        t = loc.get_tree()
        N, K = len(t['node_plane']), 9
        child = numpy.where(t['node_plane'][:, None] >= 0, t['node_child'] + K, t['node_child'])
        chain_child = numpy.array([[i + 1, N + K] for i in range(K)], dtype=numpy.int32)
        loc.set_tree(t['planes'], numpy.r_[numpy.zeros(K, dtype=numpy.int32), t['node_plane'], -1].astype(numpy.int32),
                     numpy.vstack([chain_child, child, [[-1, -1]]]).astype(numpy.int32),
                     numpy.vstack([numpy.tile([numpy.inf, 0.0], (K, 1)), t['node_tau'], [[0.0, 0.0]]]),
                     numpy.r_[numpy.zeros(K, dtype=numpy.int64), t['node_off'], t['node_off'][-1]], t['items'], t['tol'])
        got = _run(loc, k, 'tree')
    finally:
        loc.close()
    _same(got, want, k['n'], k['steps'], 'tree')
    stats = got[5]
    assert 0 < stats['fallbacks'] < stats['traj_steps']
    plane = t['planes'][0]
    if numpy.count_nonzero(plane[:-1]) == 1 and abs(plane[:-1]).max() == 1.0:     # an axis plane: s is exact, and so is the count
        a = int(numpy.flatnonzero(plane[:-1])[0])
        # trajectory p is located at the steps k <= exit_step - 1, and at k = exit_step too when that step found no region
        last = want['exit_step'] - (want['status'] != 2)
        located = numpy.arange(k['steps'])[None, :] <= last[:, None]
        assert stats['fallbacks'] == int(numpy.sum(plane[a] * want['theta'][:, :-1, a][located] - plane[-1] <= 0.0))
