"""Closed-loop simulation on the device (Solution.simulate): the per-step certificate against the batched locator and a
numpy replay of the plant, the three locators against each other, the host reference loop, disturbances, records, determinism,
stop_tol, a 10^6-trajectory run and the library's refusals."""
import warnings

import numpy
import pytest

import closed_loop_reference as ref
from ppopt_amd import _lib, closed_loop, problem_generator as pg

pytestmark = pytest.mark.gpu

_SOLVED = {}


def _solve(name):
    if name in _SOLVED:
        return _SOLVED[name]
    import bench
    from ppopt_amd.mp_solvers import mpqp_hip_combi_graph, mpqp_hip_combinatorial
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if name in ('c2', 'c2x20'):
            sol = solve_mpqp(bench.build_program(name), mpqp_algorithm.combinatorial)
        elif name == 'c3_l4':
            sol = mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4)
        elif name == 'c3_graph':
            sol = mpqp_hip_combi_graph.solve_graph(bench.build_program('c3'))
        elif name == 'mi':
            from test_export import mixed_integer_solution
            sol = mixed_integer_solution('mpMIQP_market_problem')[0]
        elif name == 'c3_merged':
            sol = _solve('c3_l4').merge_regions(outputs=[0, 1])
        else:
            raise KeyError(name)
    _SOLVED[name] = sol
    return sol


def _plant(name, sol):
    if name in ('c2', 'c2x20'):
        return pg.double_integrator_plant(5)
    if name in ('c3_l4', 'c3_graph'):
        return pg.quad_tank_plant()
    if name == 'c3_merged':
        return dict(pg.quad_tank_plant(), inputs=[0, 1])       # the merged law holds the rows x[0:2] only
    n_t = sol.theta_dim()
    rng = numpy.random.default_rng(5)
    return {'A': 0.9 * numpy.eye(n_t), 'B': rng.uniform(-0.2, 0.2, size=(n_t, 1)), 'inputs': [0]}


def _starts(sol, n, rng):
    """uniform over the box of the regions' facet centres widened by 20 % on every side: points inside and outside the solution"""
    ef, row_off, _ = sol._stacked()
    centre, _, status = _lib.facet_centres(ef, row_off)
    c = centre[(status == 0) & numpy.all(numpy.isfinite(centre), axis=1)]
    lo, hi = c.min(axis=0), c.max(axis=0)
    span = numpy.maximum(hi - lo, 1e-3)
    return rng.uniform(lo - 0.2 * span, hi + 0.2 * span, size=(n, ef.shape[1] - 1))


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


def certify(sol, res, A, B, inputs, c=None, w=None, stop_tol=None, rows=None):
    """Every recorded step of the trajectories `rows` (all: None): region = get_region_batch, u = evaluate_batch[:, inputs] and theta_{k+1} =
    the replay, bit for bit; statuses, exit steps and the NaN / -1 tails consistent with them.  Returns the status counts."""
    rows = numpy.arange(len(res.status)) if rows is None else numpy.asarray(rows)
    theta, u, region = res.theta[rows], res.u[rows], res.region[rows]
    status, ex = res.status[rows], res.exit_step[rows]
    n, K = region.shape
    assert set(numpy.unique(status).tolist()) <= {0, 1, 2, 3}
    assert numpy.all((ex >= 0) & (ex <= K))
    assert numpy.all(ex[status == 0] == K)
    taken = numpy.arange(K)[None, :] < ex[:, None]                    # steps that located a region and moved
    ps, ks = numpy.nonzero(taken)
    pts = theta[ps, ks]
    assert numpy.all(numpy.isfinite(pts))
    assert numpy.array_equal(region[ps, ks], sol.get_region_batch(pts))
    assert numpy.all(region[ps, ks] >= 0)
    x, _ = sol.evaluate_batch(pts)
    assert numpy.array_equal(_bits(u[ps, ks]), _bits(x[:, inputs]))
    wk = None if w is None else w[rows][ps, ks]
    assert numpy.array_equal(_bits(theta[ps, ks + 1]), _bits(closed_loop.replay_step(pts, u[ps, ks], A, B, c, wk)))
    # the end of every trajectory
    left = numpy.flatnonzero((status == 2))
    if len(left):
        assert numpy.all(ex[left] < K)
        assert numpy.all(sol.get_region_batch(theta[left, ex[left]]) == -1)
    bad = numpy.flatnonzero(status == 3)
    for p in bad:
        assert not numpy.all(numpy.isfinite(theta[p, ex[p]]))
    steady = numpy.zeros((n, K), dtype=bool)
    if stop_tol is not None:
        steady = numpy.all(numpy.abs(theta[:, 1:] - theta[:, :-1]) <= stop_tol, axis=2) & taken
    first = numpy.where(steady.any(axis=1), steady.argmax(axis=1) + 1, -1)
    assert numpy.array_equal(status == 1, first >= 0)
    assert numpy.all(ex[status == 1] == first[status == 1])
    after = numpy.arange(K + 1)[None, :] > ex[:, None]
    assert numpy.isnan(theta[after]).all()
    assert numpy.isnan(u[~taken]).all() and numpy.all(region[~taken] == -1)
    return numpy.bincount(status, minlength=4)


CASES = ['c2', 'c2x20', 'c3_l4', 'c3_graph', 'mi', 'c3_merged']


@pytest.mark.parametrize('name', CASES)
def test_per_step_certificate(name):
    sol = _solve(name)
    pl = _plant(name, sol)
    th0 = _starts(sol, 10_000, numpy.random.default_rng(11))
    res = sol.simulate(th0, 50, pl['A'], pl['B'], pl['inputs'])
    assert res.theta.shape == (10_000, 51, sol.theta_dim()) and res.region.dtype == numpy.int64
    counts = certify(sol, res, pl['A'], pl['B'], pl['inputs'])
    print(name, len(sol), res.stats['mode'], 'statuses', counts.tolist(), 'fallbacks', res.stats['fallbacks'],
          'crossings/step', round(res.stats['crossings_per_step'], 3))
    # a step that ends a trajectory with status 2 located too
    assert res.stats['trajectory_steps'] == int(numpy.sum(res.exit_step) + numpy.sum(res.status == 2))


def test_modes_agree_bit_for_bit():
    sol = _solve('c3_graph')
    pl = _plant('c3_graph', sol)
    th0 = _starts(sol, 10_000, numpy.random.default_rng(12))
    runs = {m: sol.simulate(th0, 50, pl['A'], pl['B'], pl['inputs'], locate=m) for m in ('scan', 'walk', 'tree')}
    assert runs['walk'].stats['mode'] == 'walk' and runs['tree'].stats['mode'] == 'tree' and runs['scan'].stats['mode'] == 'scan'
    for m in ('walk', 'tree'):
        for f in ('theta', 'u'):
            assert numpy.array_equal(_bits(getattr(runs[m], f)), _bits(getattr(runs['scan'], f))), (m, f)
        for f in ('region', 'status', 'exit_step'):
            assert numpy.array_equal(getattr(runs[m], f), getattr(runs['scan'], f)), (m, f)
    print('walk crossings/step', runs['walk'].stats['crossings_per_step'], 'fallbacks walk / tree', runs['walk'].stats['fallbacks'],
          runs['tree'].stats['fallbacks'])
    # with the tree attached, 'auto' takes it
    assert sol.simulate(th0[:100], 5, pl['A'], pl['B'], pl['inputs']).stats['mode'] == 'tree'
    small = _solve('c3_l4')
    th1 = _starts(small, 10_000, numpy.random.default_rng(13))
    a = small.simulate(th1, 50, pl['A'], pl['B'], pl['inputs'], locate='scan')
    b = small.simulate(th1, 50, pl['A'], pl['B'], pl['inputs'], locate='tree')
    assert numpy.array_equal(_bits(a.theta), _bits(b.theta)) and numpy.array_equal(a.region, b.region)
    assert numpy.array_equal(a.status, b.status) and numpy.array_equal(a.exit_step, b.exit_step)


@pytest.mark.parametrize('name', ['c2x20', 'c3_l4'])
def test_against_the_host_loop(name):
    sol = _solve(name)
    sol.materialize()
    pl = _plant(name, sol)
    th0 = _starts(sol, 256, numpy.random.default_rng(14))
    dev = sol.simulate(th0, 30, pl['A'], pl['B'], pl['inputs'])
    host = ref.simulate(sol, th0, 30, pl['A'], pl['B'], pl['inputs'])
    ef, _, _ = sol._stacked()
    tol = sol.point_location_tolerance
    near = 0
    for p in range(256):
        th = host['theta'][p]
        th = th[numpy.all(numpy.isfinite(th), axis=1)]
        if numpy.min(numpy.abs(th @ ef[:, 1:].T - ef[:, 0] - tol)) <= 1e-7:
            near += 1
            continue
        assert numpy.array_equal(dev.region[p], host['region'][p]), p
        assert dev.status[p] == host['status'][p] and dev.exit_step[p] == host['exit_step'][p], p
        ok = numpy.isfinite(host['theta'][p])
        assert numpy.array_equal(ok, numpy.isfinite(dev.theta[p]))
        assert numpy.all(numpy.abs(dev.theta[p][ok] - host['theta'][p][ok]) <= 1e-9 * (1 + numpy.abs(host['theta'][p][ok])))
    print(name, 'trajectories within 1e-7 of a region row on the host (excluded):', near)
    assert near == 0


def test_disturbances():
    sol = _solve('c3_l4')
    pl = _plant('c3_l4', sol)
    n, K = 10_000, 50
    th0 = _starts(sol, n, numpy.random.default_rng(15))
    lo, hi = numpy.full(4, -0.05), numpy.array([0.05, 0.02, 0.1, 0.0])
    box = sol.simulate(th0, K, pl['A'], pl['B'], pl['inputs'], disturbance=(lo, hi), seed=2026)
    w = closed_loop.disturbance_box(2026, n, K, lo, hi)
    arr = sol.simulate(th0, K, pl['A'], pl['B'], pl['inputs'], disturbance=w)
    for f in ('theta', 'u'):
        assert numpy.array_equal(_bits(getattr(box, f)), _bits(getattr(arr, f))), f
    assert numpy.array_equal(box.region, arr.region) and numpy.array_equal(box.status, arr.status)
    certify(sol, box, pl['A'], pl['B'], pl['inputs'], w=w)
    other = sol.simulate(th0, K, pl['A'], pl['B'], pl['inputs'], disturbance=(lo, hi), seed=2027)
    assert not numpy.array_equal(_bits(other.theta), _bits(box.theta))
    c = numpy.array([0.01, -0.02, 0.0, 0.005])
    withc = sol.simulate(th0, K, pl['A'], pl['B'], pl['inputs'], c=c, disturbance=w)
    certify(sol, withc, pl['A'], pl['B'], pl['inputs'], c=c, w=w)


def test_records_determinism_and_stop_tol():
    sol = _solve('c3_l4')
    pl = _plant('c3_l4', sol)
    th0 = _starts(sol, 10_000, numpy.random.default_rng(16))
    full = sol.simulate(th0, 50, pl['A'], pl['B'], pl['inputs'], stop_tol=1e-3)
    counts = certify(sol, full, pl['A'], pl['B'], pl['inputs'], stop_tol=1e-3)
    assert counts[1] > 0                      # the quadruple tank settles
    fin = sol.simulate(th0, 50, pl['A'], pl['B'], pl['inputs'], stop_tol=1e-3, record='final')
    assert fin.u is None and fin.region is None and fin.theta.shape == th0.shape
    assert numpy.array_equal(fin.status, full.status) and numpy.array_equal(fin.exit_step, full.exit_step)
    last = full.theta[numpy.arange(len(th0)), full.exit_step]
    assert numpy.array_equal(_bits(fin.theta), _bits(last))
    again = sol.simulate(th0, 50, pl['A'], pl['B'], pl['inputs'], stop_tol=1e-3)
    for f in ('theta', 'u'):
        assert numpy.array_equal(_bits(getattr(again, f)), _bits(getattr(full, f)))
    assert numpy.array_equal(again.region, full.region) and numpy.array_equal(again.exit_step, full.exit_step)


def test_a_million_trajectories_with_the_walk():
    sol = _solve('c3_graph')
    pl = _plant('c3_graph', sol)
    th0 = _starts(sol, 1_000_000, numpy.random.default_rng(17))
    res = sol.simulate(th0, 20, pl['A'], pl['B'], pl['inputs'], locate='walk')
    assert res.stats['mode'] == 'walk'
    rows = numpy.random.default_rng(18).choice(len(th0), size=2000, replace=False)
    certify(sol, res, pl['A'], pl['B'], pl['inputs'], rows=rows)
    print('1e6 x 20 walk: ms', res.stats['ms'], 'statuses', res.stats['status_counts'], 'fallbacks', res.stats['fallbacks'])


def test_refusals_on_the_device_path():
    sol = _solve('c3_l4')
    pl = _plant('c3_l4', sol)
    tree = sol.search_tree()
    loc = tree._locator(0)
    th0 = numpy.zeros((4, 4))
    with pytest.raises(_lib.MpcError, match='tolerance the tree was built for'):
        loc.simulate(th0, 3, pl['A'], pl['B'], pl['inputs'], tol=10 * tree.tol, tree=True)
    with pytest.raises(_lib.MpcError, match='out of range'):
        loc.simulate(th0, 3, pl['A'], pl['B'], [99, 0])
    with pytest.raises(_lib.MpcError, match='WALK'):
        loc.simulate(th0, 3, pl['A'], pl['B'], pl['inputs'], walk=True, overlapping=True)
    with pytest.raises(_lib.MpcError, match='budget'):
        loc.simulate(numpy.zeros((100_000, 4)), 100, pl['A'], pl['B'], pl['inputs'], budget=1 << 20)
    with pytest.raises(_lib.MpcError, match='finite'):
        loc.simulate(th0, 3, pl['A'], pl['B'], pl['inputs'], box=(numpy.zeros(4), numpy.full(4, numpy.inf)))
    with pytest.raises(ValueError, match='walk needs'):
        _solve('c3_l4').simulate(th0, 3, pl['A'], pl['B'], pl['inputs'], locate='walk')
