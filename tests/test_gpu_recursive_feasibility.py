"""The recursive-feasibility certificate on the device (Solution.certify_recursive_feasibility): an analytic 1-D program
with hand-computed verdicts, witnesses and margins, with and without a box disturbance; c2, c3 and a merged c3 with their plants,
every "inside" verdict checked by sampled points mapped one step, every witness image infeasible, and interior points near large
witnesses leaving too."""
import warnings

import numpy
import pytest

from ppopt_amd import MPQP_Program, invariance, problem_generator as pg
from ppopt_amd.geometry.polytope import Polytope
from ppopt_amd.geometry.polytope_operations import hit_and_run_batch
from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp

pytestmark = pytest.mark.gpu


def _one_d(a, c_max, T=10.0):
    """min u^2 s.t. |u| <= 1, |a theta + u| <= c_max, |theta| <= T: the plant theta+ = a theta + u"""
    A = numpy.array([[1.0], [-1.0], [1.0], [-1.0]])
    b = numpy.array([[1.0], [1.0], [c_max], [c_max]])
    F = numpy.array([[0.0], [0.0], [-a], [a]])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        prog = MPQP_Program(A, b, numpy.zeros((1, 1)), numpy.zeros((1, 1)), numpy.array([[2.0]]), numpy.array([[1.0], [-1.0]]),
                            numpy.array([[T], [T]]), F)
        sol = solve_mpqp(prog, mpqp_algorithm.combinatorial)
    return sol, numpy.array([[a]]), numpy.array([[1.0]])


def test_one_d_certified():
    sol, A, B = _one_d(2.0, 0.5)
    assert len(sol) == 3
    cert = sol.certify_recursive_feasibility(A, B, [0])
    assert cert.certified and cert.status.tolist() == [0, 0, 0]
    assert numpy.all(cert.margin < 0) and numpy.all(numpy.isnan(cert.witness_theta))
    assert cert.stats['lps'] == 6


def test_one_d_leaves():
    sol, A, B = _one_d(2.0, 2.0)
    cert = sol.certify_recursive_feasibility(A, B, [0])
    assert not cert.certified and cert.status.tolist() == [1, 1, 1]
    # Theta_f = |theta| <= 1.5; every region reaches theta+ = +-2.  On the unscaled rows s* = 0.2 there (u = -+1.4: 1 + 2 s = -2 + 3 s);
    # the presolved program's rows are scaled to unit norm, which changes s*: solve the margin LP of theta+ = 2 on the host
    from scipy.optimize import linprog
    A3, b2, eq, c = invariance.margin_lp_rows(sol.program, numpy.array([[2.0]]))
    want = linprog(c, A_ub=A3[0][eq == 0], b_ub=b2[0][eq == 0], bounds=[(None, None)] * len(c), method='highs').fun
    assert want > 0.1
    assert numpy.allclose(cert.margin, want, atol=1e-9, rtol=1e-9)
    assert numpy.allclose(numpy.abs(cert.witness_image[:, 0]), 2.0, atol=1e-9)
    for i, cr in enumerate(sol.critical_regions):
        th = cert.witness_theta[i]
        assert numpy.all(cr.E @ th <= cr.f.reshape(-1) + 1e-9)
        u = cr.A @ th + cr.b.reshape(-1)
        assert numpy.allclose(2.0 * th + u[0], cert.witness_image[i], atol=1e-9)


@pytest.mark.parametrize('w,ok', [(0.2, True), (0.249, True), (0.251, False), (0.3, False)])
def test_one_d_box(w, ok):
    sol, A, B = _one_d(2.0, 0.5)
    cert = sol.certify_recursive_feasibility(A, B, [0], disturbance=([-w], [w]))
    assert cert.certified == ok
    assert cert.stats['lps'] == 12
    if not ok:
        assert numpy.allclose(numpy.abs(cert.witness_image[cert.status == 1, 0]), 0.5 + w)


_SOLVED = {}


def _case(name):
    if name not in _SOLVED:
        import bench
        from ppopt_amd.mp_solvers import mpqp_hip_combinatorial
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if name == 'c2':
                _SOLVED[name] = (solve_mpqp(bench.build_program('c2'), mpqp_algorithm.combinatorial), pg.double_integrator_plant(5))
            elif name == 'c3_l4':
                _SOLVED[name] = (mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4), pg.quad_tank_plant())
            elif name == 'c3_merged':
                _SOLVED[name] = (_case('c3_l4')[0].merge_regions(outputs=[0, 1]), dict(pg.quad_tank_plant(), inputs=[0, 1]))
    return _SOLVED[name]


def _feasible(prog, pts, tol=1e-6):
    """the program is feasible at every row of pts: solve_theta_batch, and A_t theta <= b_t (the batch solves outside points too)"""
    res = prog.solve_theta_batch(pts)
    inside = numpy.all(pts @ prog.A_t.T <= prog.b_t.reshape(1, -1) + tol * (1 + numpy.abs(prog.b_t.reshape(1, -1))), axis=1)
    return numpy.array([r is not None for r in res]) & inside


@pytest.mark.parametrize('name', ['c2', 'c3_l4', 'c3_merged'])
def test_plants(name):
    sol, plant = _case(name)
    cert = sol.certify_recursive_feasibility(plant['A'], plant['B'], plant['inputs'])
    assert (cert.status != 2).all(), cert.stats
    prog = sol.program
    _, _, xlaw = sol._stacked()
    Phi, phi = invariance.closed_loop_maps(xlaw, plant['A'], plant['B'], numpy.asarray(plant['inputs']))
    inside = numpy.flatnonzero(cert.status == 0)
    rng = numpy.random.default_rng(1)
    pick = inside if len(inside) <= 200 else rng.choice(inside, 200, replace=False)
    polys = [Polytope(sol.critical_regions[i].E, sol.critical_regions[i].f) for i in pick]
    if len(polys):
        pts = hit_and_run_batch(polys, chains=8, samples=1, n_steps=50, seed=3)[:, :, 0, :]          # [k, 8, n_t]
        img = numpy.einsum('ktj,kcj->kct', Phi[pick], pts) + phi[pick][:, None, :]
        ok = _feasible(prog, img.reshape(-1, img.shape[-1]))
        if not ok.all():
            # beyond tol only: an image on the boundary of Theta_f may be refused by the QP; its margin must be tiny
            s, _, _ = invariance.margins(prog, img.reshape(-1, img.shape[-1])[~ok])
            assert numpy.all(s <= 1e-6), s.max()
    leaves = numpy.flatnonzero(cert.status == 1)
    if len(leaves):
        assert not _feasible(prog, cert.witness_image[leaves], tol=0.0).any() or numpy.all(cert.margin[leaves] <= 1e-5)
        big = [i for i in leaves if cert.margin[i] > 1e-4]
        for i in big[:20]:
            cr = sol.critical_regions[i]
            from ppopt_amd.utils.chebyshev_ball import chebyshev_ball
            cb = chebyshev_ball(cr.E, cr.f)
            centre = numpy.asarray(cb.sol).reshape(-1)[:-1] if cb is not None else cert.witness_theta[i]
            th = cert.witness_theta[i] + 1e-6 * (centre - cert.witness_theta[i]) / max(1e-12, numpy.linalg.norm(centre - cert.witness_theta[i]))
            nxt = Phi[i] @ th + phi[i]
            assert not _feasible(prog, nxt[None], tol=0.0)[0]
