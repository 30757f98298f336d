"""The CPU references of tests/theta_reference.py checked on their own: the certificate path against the enumeration path on
random small QPs, the certificate against deliberately wrong answers, the feasibility margin on sets whose emptiness is known,
and the LP / MILP / MIQP references against answers known in closed form."""
import numpy
import pytest

import theta_reference as tr


def random_qp(rng, nc, nx, n_eq):
    M = rng.standard_normal((nx, nx))
    Q = M @ M.T + 0.5 * numpy.eye(nx)
    A = rng.standard_normal((nc, nx))
    x0 = rng.standard_normal(nx)
    r = A @ x0 + numpy.concatenate([numpy.zeros(n_eq), rng.uniform(-0.5, 1.0, nc - n_eq)])
    g = 3.0 * rng.standard_normal(nx)
    return Q, g, A, r


def test_certificate_agrees_with_enumeration():
    rng = numpy.random.default_rng(11)
    n_feasible = n_infeasible = 0
    for k in range(50):
        nx = int(rng.integers(1, 6))
        nc = int(rng.integers(1, 9))
        n_eq = int(rng.integers(0, min(nc, nx - 1) + 1)) if nx > 1 else 0
        Q, g, A, r = random_qp(rng, nc, nx, n_eq)
        if k % 7 == 3:
            r[n_eq:] -= 3.0                      # often empty
        verdict = tr.feasibility_verdict(A, r, n_eq)
        e = tr.qp_enumerate(Q, g, A, r, n_eq)
        if verdict == 'edge':
            continue
        assert (e is not None) == (verdict == 'feasible'), (k, verdict)
        if e is None:
            n_infeasible += 1
            continue
        n_feasible += 1
        assert e.ok and e.primal_margin >= -1e-12 and e.dual_margin >= -1e-12
        # the certificate of the enumeration's active set, claimed again from the slacks (what a device reports)
        s = (r - A @ e.x) / (numpy.abs(r) + numpy.abs(A) @ numpy.abs(e.x))
        act = numpy.abs(s) <= 1e-12
        c = tr.qp_certificate(Q, g, A, r, n_eq, act, order_hint=e.lam)
        assert c.ok, c.reasons
        err = tr.compare_qp(c, Q, g, A, e.x, e.lam, 1e-12)
        assert err['x'] <= 1e-12 and err['lam'] <= 1e-10 and err['obj'] <= 1e-12, (k, err)
        # and the KKT conditions themselves, from scratch
        assert numpy.allclose(Q @ e.x + g + A.T @ e.lam, 0.0, atol=1e-10 * (1 + numpy.abs(g).max()))
    assert n_feasible >= 30 and n_infeasible >= 3


def _strict_case():
    """A QP whose optimum has two strongly active rows (multipliers well away from zero)."""
    Q = numpy.diag([1.0, 2.0, 3.0])
    g = numpy.array([-4.0, -4.0, 1.0])
    A = numpy.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 1.0], [0.0, 0.0, -1.0]])
    r = numpy.array([1.0, 1.0, 10.0, 5.0])
    return Q, g, A, r


def test_certificate_rejects_wrong_answers():
    Q, g, A, r = _strict_case()
    e = tr.qp_enumerate(Q, g, A, r, 0)
    assert e is not None and list(numpy.flatnonzero(e.lam > 1e-9)) == [0, 1]
    act = numpy.array([True, True, False, False])
    good = tr.qp_certificate(Q, g, A, r, 0, act)
    assert good.ok
    tol = tr.qp_tolerance(good)
    ok = tr.compare_qp(good, Q, g, A, e.x, e.lam, tol)
    assert max(ok['x'], ok['lam'], ok['obj']) <= tol
    # x moved by 1e-8 relative
    moved = tr.compare_qp(good, Q, g, A, e.x * (1 + 1e-8), e.lam, tol)
    assert moved['x'] > tol
    # a dropped active row: the KKT point of the rest violates it
    dropped = tr.qp_certificate(Q, g, A, r, 0, numpy.array([True, False, False, False]))
    assert not dropped.ok and dropped.primal_margin < -1e-3
    # a flipped multiplier sign
    flipped = tr.compare_qp(good, Q, g, A, e.x, e.lam * numpy.array([-1.0, 1.0, 1.0, 1.0]), tol)
    assert flipped['lam'] > tol
    # a row claimed active that must not be (its multiplier would be negative)
    extra = tr.qp_certificate(Q, g, A, r, 0, numpy.array([True, True, False, True]))
    assert not extra.ok and extra.dual_margin < -1e-3


def test_certificate_weakly_active_and_dependent_rows():
    Q, g, A, r = _strict_case()
    # a duplicate of row 0 and a row parallel to row 1 scaled by 2: both weakly active at the optimum
    A2 = numpy.vstack([A, A[0], 2.0 * A[1]])
    r2 = numpy.concatenate([r, [r[0], 2.0 * r[1]]])
    e = tr.qp_enumerate(Q, g, A2, r2, 0)
    act = numpy.array([True, True, False, False, True, True])
    c = tr.qp_certificate(Q, g, A2, r2, 0, act)
    assert c.ok and len(c.rows) == 2
    assert numpy.allclose(c.x, e.x, rtol=0, atol=1e-14)
    # a dependent but consistent equality row
    Ae = numpy.vstack([[1.0, 1.0, 0.0], [0.0, 1.0, 1.0], [1.0, 2.0, 1.0], A])
    re = numpy.concatenate([[0.5, 0.25, 0.75], r])
    e = tr.qp_enumerate(Q, g, Ae, re, 3)
    assert e is not None and e.ok
    assert tr.feasibility_verdict(Ae, re, 3) == 'feasible'
    re_bad = re.copy()
    re_bad[2] += 1e-3
    assert tr.qp_enumerate(Q, g, Ae, re_bad, 3) is None
    assert tr.feasibility_verdict(Ae, re_bad, 3) == 'infeasible'


def test_feasibility_certificate_on_known_sets():
    # the box |x_i| <= w: nonempty for w > 0, a single point for w = 0 (knife-edge), empty for w < 0
    A = numpy.vstack([numpy.eye(3), -numpy.eye(3)])
    for w, want in ((1.0, 'feasible'), (1e-3, 'feasible'), (0.0, 'edge'), (-1e-9, 'edge'), (-1e-3, 'infeasible')):
        assert tr.feasibility_verdict(A, numpy.full(6, w), 0) == want, w
    assert abs(tr.feasibility_margin(A, numpy.full(6, 0.25), 0) - 0.25) <= 1e-12
    # rows scaled by 1e6 measure the same distance
    assert abs(tr.feasibility_margin(1e6 * A, numpy.full(6, 0.25e6), 0) - 0.25) <= 1e-9
    # x1 + x2 = 3 within the box of half-width 1: empty; = 1.5: not
    Ae = numpy.vstack([[1.0, 1.0, 0.0], A])
    assert tr.feasibility_verdict(Ae, numpy.concatenate([[3.0], numpy.ones(6)]), 1) == 'infeasible'
    assert tr.feasibility_verdict(Ae, numpy.concatenate([[1.5], numpy.ones(6)]), 1) == 'feasible'
    # inconsistent equalities
    assert tr.feasibility_margin(numpy.array([[1.0, 0.0], [1.0, 0.0]]), numpy.array([0.0, 1.0]), 2) == -numpy.inf


def test_lp_and_milp_references():
    A = numpy.array([[1.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    assert tr.lp_reference(A, [4.0, 0.0, 0.0], [-1.0, -2.0], [False] * 3) == (0, -8.0)
    assert tr.lp_reference(A, [4.0, 0.0, 0.0], [1.0, -2.0], [False] * 3)[0] == 0
    assert tr.lp_reference(A, [-1.0, 0.0, 0.0], [1.0, 1.0], [False] * 3)[0] == 1
    assert tr.lp_reference(A[1:], [0.0, 0.0], [-1.0, 0.0], [False] * 2)[0] == 2
    # x0 binary, x1 free: min -x0 - x1 s.t. x1 <= 0.5 + 0.25 x0 ... as x1 - 0.25 x0 <= 0.5
    st, f = tr.milp_reference(numpy.array([[-0.25, 1.0]]), [0.5], [-1.0, -1.0], [False], [0])
    assert st == 0 and abs(f + 1.75) <= 1e-12


def test_miqp_brute_force_small():
    # min 1/2 x^2 + 1/2 y - x  s.t.  x <= y  (y binary): y = 0 -> x = 0, obj 0; y = 1 -> x = 1, obj -1/2 + 1/2 = 0 (a tie)
    Q = numpy.diag([1.0, 0.0])
    c = numpy.array([-1.0, 0.5])
    A = numpy.array([[1.0, -1.0]])
    best, objs = tr.miqp_brute_force(Q, c, numpy.zeros((2, 1)), A, [0.0], numpy.zeros((1, 1)), 0, [1], [[0.0], [1.0]], [0.0])
    assert abs(objs[0]) <= 1e-15 and abs(objs[1]) <= 1e-15 and best == 0.0
    # with a pure-binary check row y >= 1 only the second fixation remains
    A2 = numpy.vstack([A, [0.0, -1.0]])
    best, objs = tr.miqp_brute_force(Q, c, numpy.zeros((2, 1)), A2, [0.0, -1.0], numpy.zeros((2, 1)), 0, [1], [[0.0], [1.0]], [0.0])
    assert objs[0] is None and abs(objs[1]) <= 1e-15


def test_solve_theta_batch_raises_at_the_iteration_limit(monkeypatch):
    """A point whose Lemke run stopped at the iteration limit has no answer: solve_theta_batch raises instead of returning None
    (which would read as "infeasible").  The device call is replaced by a stub returning that status."""
    from ppopt_amd import MPQP_Program, _lib
    Q, g, A, r = _strict_case()
    prog = MPQP_Program(A, r.reshape(-1, 1), g.reshape(-1, 1), numpy.zeros((3, 1)), Q, numpy.array([[1.0], [-1.0]]),
                        numpy.ones((2, 1)), numpy.zeros((4, 1)), post_process=False, _diagnostics=False)

    class Stub:
        def qp_solve_batch(self, th):
            m = len(th)
            return numpy.array([0, 3] * m)[:m].astype(numpy.int32), numpy.zeros((m, 3)), numpy.zeros((m, 4)), numpy.zeros((m, 4), bool)
    monkeypatch.setattr(prog, 'engine', lambda *a, **k: Stub())
    assert prog.solve_theta_batch(numpy.zeros((1, 1)))[0] is not None
    with pytest.raises(_lib.MpcError, match='iteration limit'):
        prog.solve_theta_batch(numpy.zeros((2, 1)))
