"""Mixed-integer programs at parameter points on the MI355X: MPMIQP_Program.solve_theta(_batch) (mpc_miqp_solve_batch, one LCP
per (point, fixation) pair), MPMILP_Program.solve_theta_batch (LP batches), and Solution.verify_theta / verify_solution of
mixed-integer solutions, against the reference's values (tests/golden/mi_*.npz), the explicit solutions and the per-fixation
loop of substituted QPs."""
import glob
import os

import numpy
import pytest

from test_gpu_mi import build, _load

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MIQP = ['simple_mpMIQP', 'mpMIQP_market_problem', 'rand_4_2_8_b3_s1', 'rand_6_3_12_b5_s0']
MILP = [os.path.basename(p)[3:-4] for p in sorted(glob.glob(os.path.join(GOLDEN, 'mi_*.npz')))
        if str(numpy.load(p)['cls']) == 'MPMILP_Program']


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def _near_boundary(prog, th, eps=1e-6):
    """Does the feasibility of the program change within eps of th (along the axes)?"""
    nt = len(th)
    pts = numpy.vstack([th + eps * s * numpy.eye(nt)[k] for k in range(nt) for s in (1.0, -1.0)])
    here = prog.solve_theta_batch(th.reshape(1, -1))[0] is not None
    return any((r is not None) != here for r in prog.solve_theta_batch(pts))


def _inside(prog, th):
    return bool(numpy.all(prog.A_t @ th.reshape(-1, 1) <= prog.b_t + 1e-12))


def test_milp_goldens_present():
    assert len(MILP) == 9


@pytest.mark.parametrize('name', MIQP)
def test_miqp_reference_values(name):
    g = _load(name)
    prog = build(g)
    res = prog.solve_theta_batch(g['T_theta'])
    for th, ok, obj, r in zip(g['T_theta'], g['T_ok'], g['T_obj'], res):
        if ok:
            assert r is not None and _rel(r.obj, float(obj)) <= 1e-8, (name, th)
        elif _inside(prog, th) and r is not None:
            assert _near_boundary(prog, th), (name, th)


def _theta_box(prog, fallback=None):
    """Bounding box of the parameter set (2 n_theta LPs); ``fallback`` [k, n_theta] points whose range, widened, serves where the
    set is unbounded."""
    nt = prog.num_t()
    lo, hi = numpy.zeros(nt), numpy.zeros(nt)
    for j in range(nt):
        for sign, out in ((1.0, lo), (-1.0, hi)):
            c = numpy.zeros((nt, 1))
            c[j, 0] = sign
            r = prog.solver.solve_lp(c, prog.A_t, prog.b_t)
            if r is None:
                span = fallback.max(axis=0) - fallback.min(axis=0)
                return fallback.min(axis=0) - 0.1 * span, fallback.max(axis=0) + 0.1 * span
            out[j] = sign * r.obj
    return lo, hi


def _explicit_cases():
    return [('golden', n) for n in MIQP] + [('generated', s) for s in (0, 1, 2)]


@pytest.mark.parametrize('kind,key', _explicit_cases(), ids=[f'{k}-{v}' for k, v in _explicit_cases()])
def test_miqp_agrees_with_the_explicit_solution(kind, key):
    import warnings
    from ppopt_amd import MPMIQP_Program
    from ppopt_amd.mp_solvers.solve_mpmiqp import solve_mpmiqp
    from ppopt_amd.problem_generator import generate_mpmiqp_data
    fallback = None
    if kind == 'golden':
        g = _load(key)
        prog, fallback = build(g), g['T_theta']
    else:
        d = generate_mpmiqp_data(6, 3, 12, 4, key)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            prog = MPMIQP_Program(d['A'], d['b'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], d['F'], d['binary_indices'])
    sol = solve_mpmiqp(prog, num_cores=1)
    lo, hi = _theta_box(prog, fallback)
    pts = numpy.random.default_rng(7).uniform(lo, hi, (2000, prog.num_t()))
    pts = pts[[_inside(prog, p) for p in pts]]
    x, region = sol.evaluate_batch(pts)
    det = prog.solve_theta_batch(pts)
    compared = 0
    for p, th in enumerate(pts):
        if region[p] >= 0 and det[p] is not None:
            t = th.reshape(-1, 1)
            obj = prog.evaluate_objective(x[p].reshape(-1, 1), t)
            assert _rel(obj, det[p].obj) <= 1e-8, (key, th)
            compared += 1
        elif (region[p] >= 0) != (det[p] is not None):
            assert _near_boundary(prog, th), (key, th)
    assert compared > 0


def test_miqp_agrees_with_the_per_leaf_loop():
    g = _load('rand_6_3_12_b5_s0')
    prog = build(g)
    lo, hi = _theta_box(prog, g['T_theta'])
    pts = numpy.random.default_rng(3).uniform(lo, hi, (500, prog.num_t()))
    leaves = prog.feasible_combinations()
    objs = numpy.full((len(pts), len(leaves)), numpy.inf)
    xs = numpy.full((len(pts), len(leaves), len(prog.cont_indices)), numpy.nan)
    for l, y in enumerate(leaves):
        sub = prog.generate_substituted_problem(y, deferred=True)
        for p, r in enumerate(sub.solve_theta_batch(pts)):
            if r is not None and numpy.all(sub.A_t @ pts[p].reshape(-1, 1) <= sub.b_t):
                objs[p, l], xs[p, l] = r.obj, r.sol
    got = prog.solve_theta_batch(pts)
    compared = 0
    for p in range(len(pts)):
        best = int(numpy.argmin(objs[p]))
        if not numpy.isfinite(objs[p, best]):
            assert got[p] is None or _near_boundary(prog, pts[p])
            continue
        assert got[p] is not None
        assert _rel(got[p].obj, objs[p, best]) <= 1e-9
        second = numpy.partition(objs[p], 1)[1] if len(leaves) > 1 else numpy.inf
        if second - objs[p, best] > 1e-8 * max(1.0, abs(objs[p, best])):
            y = got[p].sol[prog.binary_indices]
            assert numpy.array_equal(y, numpy.asarray(leaves[best], dtype=float))
            numpy.testing.assert_allclose(got[p].sol[prog.cont_indices], xs[p, best], atol=1e-7, rtol=0)
            compared += 1
    assert compared > 0


@pytest.mark.parametrize('name', MIQP + MILP)
def test_solve_theta_is_the_batch_entry_bit_for_bit(name):
    g = _load(name)
    prog = build(g)
    th = g['T_theta'][:12]
    batch = prog.solve_theta_batch(th)
    for t, r in zip(th, batch):
        one = prog.solve_theta(t.reshape(-1, 1))
        assert (one is None) == (r is None), (name, t)
        if one is not None:
            assert one.obj == r.obj and numpy.array_equal(one.sol, r.sol) and numpy.array_equal(one.slack, r.slack), (name, t)
            assert numpy.array_equal(one.active_set, r.active_set)


@pytest.mark.parametrize('name', MILP)
def test_milp_batch_reference_values(name):
    g = _load(name)
    prog = build(g)
    res = prog.solve_theta_batch(g['T_theta'])
    for th, ok, obj, r in zip(g['T_theta'], g['T_ok'], g['T_obj'], res):
        if ok:
            assert r is not None and _rel(r.obj, float(obj)) <= 1e-8, (name, th)


@pytest.mark.parametrize('name', ['rand_4_2_8_b3_s1', 'mpMILP_market_problem'])
def test_chunked_batches_are_bit_identical(name, monkeypatch):
    from ppopt_amd.solver import Solver
    g = _load(name)
    prog = build(g)
    th = g['T_theta']
    whole = prog.solve_theta_batch(th)
    monkeypatch.setattr(Solver, 'MILP_BATCH_BYTES', 500)     # a few points per device call
    parts = prog.solve_theta_batch(th)
    for a, b in zip(whole, parts):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.obj == b.obj and numpy.array_equal(a.sol, b.sol)


@pytest.mark.parametrize('name', ['simple_mpMIQP', 'rand_4_2_8_b3_s1', 'mpMILP_1d', 'acevedo_mpmilp'])
def test_mixed_integer_solutions_verify(name):
    from ppopt_amd.mp_solvers.solve_mpmiqp import solve_mpmiqp
    g = _load(name)
    prog = build(g)
    sol = solve_mpmiqp(prog, num_cores=1)
    for th in g['T_theta']:
        assert sol.verify_theta(th.reshape(-1, 1)), (name, th)
    assert sol.verify_solution()


@pytest.mark.parametrize('name', ['simple_mpMIQP', 'acevedo_mpmilp'])
def test_a_wrong_mixed_integer_region_fails_verification(name):
    from ppopt_amd.mp_solvers.solve_mpmiqp import solve_mpmiqp
    prog = build(_load(name))
    sol = solve_mpmiqp(prog, num_cores=1)
    # one region made wrong: its law shifted by 1e-3, in the direction that lowers its objective at its own centre.  Verification is
    # by objective (the reference's rule), so only a region whose objective moves there by more than the tolerance can be caught:
    # the first such region that is the one located at its centre is taken (at a stationary point a shift moves the objective to
    # second order only; with overlaps a region may be dominated at its own centre)
    centres, _ = sol.chebyshev_centres()
    located = sol.get_region_batch(centres)
    for i, (cr, c) in enumerate(zip(sol.critical_regions, centres)):
        if located[i] != i:
            continue
        th, b0 = c.reshape(-1, 1), cr.b
        base = prog.evaluate_objective(cr.evaluate(th), th)
        lows = []
        for shift in (1e-3, -1e-3):
            cr.b = b0 + shift
            lows.append((prog.evaluate_objective(cr.evaluate(th), th), shift))
        cr.b = b0
        low, shift = min(lows)
        if base - low > 1e-4 * (1.0 + abs(base)):
            cr.b = b0 + shift
            sol._locator_key = None
            assert not sol.verify_solution()
            return
    pytest.fail('no region whose objective a shift of 1e-3 moves')
