"""Hit-and-run on the MI355X (mpc_hit_and_run, k_hit_and_run) against the CPU replay of the chain (tests/hit_and_run_reference.py),
its determinism and statuses, the distribution of its samples, and Solution.sample_check on small solved programs."""
import warnings

import numpy
import pytest

import hit_and_run_reference as hr
from ppopt_amd import _lib
from ppopt_amd.geometry import DEFAULT_N_STEPS, Polytope, hit_and_run, hit_and_run_batch, sample_program_theta_space

pytestmark = pytest.mark.gpu


def _random_polytope(n, m, seed, sparse=False):
    """A bounded polytope {A x <= b} with m rows around the origin (a box of 2n rows plus random rows; sparse: 2 nonzeros each)."""
    rng = numpy.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    if sparse:
        keep = numpy.zeros((m, n), dtype=bool)
        for i in range(m):
            keep[i, rng.choice(n, size=min(2, n), replace=False)] = True
        A = numpy.where(keep, A, 0.0)
    Ab, bb = hr.box(-numpy.ones(n), numpy.ones(n))
    k = max(0, m - 2 * n)
    A = numpy.vstack([Ab * rng.uniform(0.5, 2.0, (2 * n, 1)), A[:k]])
    b = numpy.concatenate([rng.uniform(0.5, 2.0, 2 * n), rng.uniform(0.3, 1.5, k)])
    return A[:max(m, 2 * n)], b[:max(m, 2 * n)]


def _bbox_width(A, b):
    from scipy.optimize import linprog
    n = A.shape[1]
    w = 0.0
    for j in range(n):
        c = numpy.zeros(n); c[j] = 1.0
        lo = linprog(c, A_ub=A, b_ub=b, bounds=[(None, None)] * n).fun
        hi = -linprog(-c, A_ub=A, b_ub=b, bounds=[(None, None)] * n).fun
        w = max(w, hi - lo)
    return w


CASES = [(1, 2, False), (2, 8, False), (3, 12, True), (8, 40, False), (10, 128, True), (16, 64, False), (17, 80, True), (33, 128, False),
         (64, 256, False), (8, 256, True)]


@pytest.mark.parametrize('n, m, sparse', CASES)
def test_chains_match_the_cpu_reference(n, m, sparse):
    A, b = _random_polytope(n, m, seed=100 + n + m, sparse=sparse)
    chains, samples, steps, seed = 96, 4, 8, 0x1234567890abcdef
    start = numpy.zeros((1, n))
    got, st = _lib.hit_and_run(numpy.array([0, len(b)]), numpy.hstack([b[:, None], A]), start, chains, samples, steps, seed)
    want, wst = hr.chains(A, b, start[0], chains, samples, steps, seed)
    assert (st[0] == 0).all() and (wst == 0).all()
    tol = 1e-9 * _bbox_width(A, b)
    err = numpy.max(numpy.abs(got[0] - want), axis=(1, 2))
    assert numpy.max(err) <= tol, (numpy.argmax(err), numpy.max(err), tol)
    assert numpy.max(got[0].reshape(-1, n) @ A.T - b) <= 1e-12 * (1 + numpy.abs(b).max())


def test_determinism_and_launch_shape_independence():
    A, b = _random_polytope(6, 30, seed=1)
    ab, off, start = numpy.hstack([b[:, None], A]), numpy.array([0, len(b)]), numpy.zeros((1, 6))
    a1, _ = _lib.hit_and_run(off, ab, start, 10, 2, 16, 77)
    a2, _ = _lib.hit_and_run(off, ab, start, 10, 2, 16, 77)
    assert numpy.array_equal(a1, a2)
    big, _ = _lib.hit_and_run(off, ab, start, 100_000, 2, 16, 77)
    assert numpy.array_equal(big[0, :10], a1[0])


def test_batch_with_unequal_row_counts_equals_one_by_one():
    polys = [_random_polytope(4, m, seed=m) for m in (8, 23, 9, 64)]
    starts = numpy.zeros((4, 4))
    off = numpy.concatenate([[0], numpy.cumsum([len(b) for _, b in polys])])
    ab = numpy.vstack([numpy.hstack([b[:, None], A]) for A, b in polys])
    got, st = _lib.hit_and_run(off, ab, starts, 70, 3, 5, 9)
    assert (st == 0).all()
    for p, (A, b) in enumerate(polys):
        # alone, polytope p is polytope 0: its chains have other global ids, so replay those with the reference's ids instead
        want, _ = hr.chains(A, b, starts[p], 70, 3, 5, 9, p=p)
        assert numpy.max(numpy.abs(got[p] - want)) <= 1e-9 * _bbox_width(A, b)
        alone, _ = _lib.hit_and_run(numpy.array([0, len(b)]), numpy.hstack([b[:, None], A]), starts[p:p + 1], 70 * (p + 1), 3, 5, 9)
        # chain g = p * 70 + k of the batch is chain g of a one-polytope run with (p + 1) * 70 chains
        assert numpy.array_equal(got[p], alone[0, p * 70:(p + 1) * 70])


def test_statuses_and_neighbours():
    box_A, box_b = hr.box(numpy.zeros(3), numpy.ones(3))
    half_A, half_b = numpy.array([[1.0, 0.0, 0.0]]), numpy.array([1.0])
    half2_A, half2_b = numpy.array([[0.0, -1.0, 0.0]]), numpy.array([1.0])
    polys = [(box_A, box_b), (half_A, half_b), (box_A, box_b), (half2_A, half2_b), (box_A, box_b)]
    starts = numpy.array([[0.5] * 3, [0.0] * 3, [2.0, 0.5, 0.5], [0.0] * 3, [0.5] * 3])
    off = numpy.concatenate([[0], numpy.cumsum([len(b) for _, b in polys])])
    ab = numpy.vstack([numpy.hstack([b[:, None], A]) for A, b in polys])
    out, st = _lib.hit_and_run(off, ab, starts, 5, 2, 7, 3)
    assert st.tolist() == [[0] * 5, [2] * 5, [1] * 5, [2] * 5, [0] * 5]
    assert numpy.isnan(out[1:4]).all() and numpy.isfinite(out[[0, 4]]).all()
    want, _ = hr.chains(box_A, box_b, starts[4], 5, 2, 7, 3, p=4)
    assert numpy.max(numpy.abs(out[4] - want)) <= 1e-12
    # a slab has finite chords in almost every direction (status 0 by the chain's rule): hit_and_run_batch refuses it by its rank
    slab = Polytope(numpy.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]]), numpy.array([1.0, 1.0]))
    with pytest.raises(_lib.MpcError, match='unbounded'):
        hit_and_run_batch(slab, starts=numpy.zeros((1, 3)))
    with pytest.raises(_lib.MpcError, match='unbounded'):
        hit_and_run_batch(Polytope(half_A, half_b), starts=numpy.zeros((1, 3)))


# ---- distribution at the default step count ---------------------------------------------------------------------------------
N_GPU = 20_000


def test_distribution_unit_box_and_rotated_box():
    A, b = hr.box(numpy.zeros(8), numpy.ones(8))
    X = hit_and_run_batch(Polytope(A, b), chains=N_GPU, seed=11)[:, 0]
    assert max(hr.check_uniform_box(X, 0.0, 1.0)) <= 1.0
    assert numpy.max(X @ A.T - b) <= 0
    R = hr.rotation(8, 2)
    X = hit_and_run_batch(Polytope(A @ R.T, b), chains=N_GPU, seed=12)[:, 0]
    assert numpy.max(X @ (A @ R.T).T - b) <= 1e-15
    assert max(hr.check_uniform_box(X @ R, 0.0, 1.0)) <= 1.0


def test_distribution_simplex_and_elongated_box():
    A, b = hr.simplex(8)
    X = hit_and_run_batch(Polytope(A, b), chains=N_GPU, seed=13)[:, 0]
    assert numpy.max(X @ A.T - b) <= 1e-15
    assert hr.check_simplex(X) <= 1.0
    # started at the centre: the Chebyshev centre of an elongated box is not unique, and the LP may return one a radius from an end
    hi = numpy.r_[10.0, numpy.ones(7)]
    A, b = hr.box(numpy.zeros(8), hi)
    X = hit_and_run_batch(Polytope(A, b), starts=hi[None] / 2, chains=N_GPU, seed=14)[:, 0]
    assert max(hr.check_uniform_box(X, 0.0, hi)) <= 1.0


def test_distribution_hexagon():
    A, b = hr.hexagon()
    X = hit_and_run_batch([Polytope(A, b)], chains=N_GPU, samples=2, seed=15)      # two samples per chain, both tested
    assert numpy.max(X.reshape(-1, 2) @ A.T - b) <= 1e-15
    for q in range(2):
        stat, limit = hr.chi2_cells(hr.hexagon_cells(X[0, :, q]), 12)
        assert stat <= limit, (q, stat, limit)


def test_single_chain_interface_and_default():
    A, b = hr.box(numpy.zeros(2), numpy.ones(2))
    x = hit_and_run(Polytope(A, b), numpy.array([[0.5], [0.5]]), n_steps=20, seed=4)
    assert x.shape == (2, 1) and numpy.all(A @ x <= b.reshape(-1, 1))
    assert hit_and_run(Polytope(A, b), numpy.array([0.5, 0.5])).shape == (2, 1)     # unseeded
    assert DEFAULT_N_STEPS >= 100
    with pytest.raises(_lib.MpcError, match='not full dimensional'):
        hit_and_run_batch(Polytope(numpy.vstack([A, [[1.0, 0.0], [-1.0, 0.0]]]), numpy.r_[b, 0.5, -0.5]))
    with pytest.raises(_lib.MpcError, match='empty'):
        hit_and_run_batch(Polytope(numpy.vstack([A, [[1.0, 0.0], [-1.0, 0.0]]]), numpy.r_[b, -2.0, -2.0]))
    with pytest.raises(_lib.MpcError, match='unbounded'):
        hit_and_run_batch(Polytope(numpy.array([[1.0, 0.0]]), numpy.array([1.0])))


# ---- Solution.sample_check --------------------------------------------------------------------------------------------------
def _mpqp(seed=3):
    from ppopt_amd import MPQP_Program, problem_generator as pg
    d = pg.generate_mpqp_data(4, 2, 10, seed)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return MPQP_Program(d['A'], d['b'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], d['F'])


def _solve(prog, **kw):
    from ppopt_amd.mp_solvers import mpqp_hip_combinatorial
    return mpqp_hip_combinatorial.solve(prog, **kw).materialize()


def test_sample_check_intact_solution():
    prog = _mpqp()
    sol = _solve(prog)
    assert len(sol) >= 4 and sol.verify_solution()
    rep = sol.sample_check(num_samples=20_000, per_region=16)
    assert rep.ok, rep
    assert rep.n_uncovered == 0 and rep.n_wrong == 0 and rep.failing_regions == [] and rep.covered_fraction == 1.0
    assert rep.n_regions_sampled == len(sol) and rep.max_x_err <= 1e-6


def test_sample_check_finds_a_missing_region():
    from ppopt_amd.solution import Solution
    prog = _mpqp()
    sol = _solve(prog)
    _, radii = sol.chebyshev_centres()
    big = int(numpy.argmax(radii))
    gone = sol.critical_regions[big]
    cut = Solution(prog, [r for i, r in enumerate(sol.critical_regions) if i != big])
    rep = cut.sample_check(num_samples=20_000, per_region=4)
    assert not rep.ok and rep.n_uncovered > 0 and rep.covered_fraction < 1.0
    E, f = numpy.asarray(gone.E), numpy.asarray(gone.f).reshape(-1)
    assert numpy.all(rep.uncovered_points @ E.T - f <= 1e-6)


def test_sample_check_flags_a_wrong_law():
    from ppopt_amd.solution import Solution
    prog = _mpqp()
    sol = _solve(prog)
    _, radii = sol.chebyshev_centres()
    j = int(numpy.argsort(radii)[len(radii) // 2])
    cr = sol.critical_regions[j]
    cr.b = numpy.asarray(cr.b, dtype=float) + 1e-3
    rep = Solution(prog, list(sol.critical_regions)).sample_check(num_samples=20_000, per_region=8)
    assert rep.failing_regions == [j] and rep.n_wrong > 0 and not rep.ok


def test_sample_check_partial_solve_reports_uncovered_points():
    prog = _mpqp(seed=5)
    full = _solve(prog)
    part = _solve(prog, max_levels=1)
    assert len(part) < len(full)
    rep = part.sample_check(num_samples=20_000, per_region=4)
    assert rep.n_uncovered > 0 and not rep.ok and rep.failing_regions == []


def test_sample_check_mplp_and_mixed_integer_goldens():
    from conftest import load_golden
    from ppopt_amd import Solver
    from ppopt_amd.mp_solvers.solve_mpmiqp import solve_mpmiqp
    from test_gpu_mi import _load, build
    from test_host_logic import build_program
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    lp = build_program(load_golden('mplp_rand_4_2_10_s0'), Solver())
    sol = solve_mpqp(lp, mpqp_algorithm.combinatorial)
    rep = sol.sample_check(num_samples=20_000, per_region=8)
    assert rep.ok, rep
    mi = solve_mpmiqp(build(_load('bard_mpMILP_adapted')), num_cores=1)
    rep = mi.sample_check(num_samples=5_000, per_region=8)
    assert rep.ok, rep


def test_sample_check_open_theta_raises():
    import copy
    from ppopt_amd.solution import Solution
    prog = _mpqp()
    sol = _solve(prog)
    open_prog = copy.copy(prog)
    open_prog.A_t, open_prog.b_t = numpy.array([[1.0, 0.0]]), numpy.array([[1.0]])     # a half-plane of parameters
    with pytest.raises(_lib.MpcError, match='parameter set'):
        Solution(open_prog, sol.critical_regions).sample_check(num_samples=100)
    with pytest.raises(_lib.MpcError, match='parameter set'):
        sample_program_theta_space(open_prog, 10)
