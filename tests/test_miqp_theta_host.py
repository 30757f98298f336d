"""Host assembly of the MIQP at a parameter point (MPMIQP_Program.theta_blocks): the blocks the device kernel of
mpc_miqp_solve_batch works from must reproduce the substituted continuous program of every fixation.  No device: the
constructor's LPs go to a stand-in, the leaves are chosen here."""
import itertools
import os
import warnings

import numpy
import pytest

from ppopt_amd.solver import Solver

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MIQP_GOLDENS = ['simple_mpMIQP', 'mpMIQP_market_problem', 'rand_4_2_8_b3_s1', 'rand_6_3_12_b5_s0']


class NoLP(Solver):         # the constructor's presolve is not what is tested here
    def solve_lp_batch(self, c, A, b, equality_sets):
        return [object()] * len(equality_sets)


def _program(A, b, c, H, Q, A_t, b_t, F, bins, **kw):
    from ppopt_amd import MPMIQP_Program
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return MPMIQP_Program(A, b, c, H, Q, A_t, b_t, F, bins, solver=NoLP(), post_process=False, **kw)


def _golden(name):
    g = numpy.load(os.path.join(GOLDEN, f'mi_{name}.npz'))
    kw = {k: g['raw_' + k] for k in ('c_c', 'c_t', 'Q_t') if 'raw_' + k in g.files}
    if 'raw_equality_indices' in g.files:
        kw['equality_indices'] = g['raw_equality_indices'].tolist()
    return _program(g['raw_A'], g['raw_b'], g['raw_c'], g['raw_H'], g['raw_Q'], g['raw_A_t'], g['raw_b_t'], g['raw_F'],
                    g['raw_binary_indices'].tolist(), **kw)


def _generated(x=4, t=2, m=10, nb=3, seed=3):
    from ppopt_amd.problem_generator import generate_mpmiqp_data
    d = generate_mpmiqp_data(x, t, m, nb, seed)
    return _program(d['A'], d['b'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], d['F'], d['binary_indices'])


def _programs():
    return [(n, _golden(n)) for n in MIQP_GOLDENS] + [('generated', _generated())]


def _z(theta, y):
    return numpy.concatenate([[1.0], numpy.ravel(theta), numpy.ravel(y)])


@pytest.mark.parametrize('name,prog', _programs(), ids=[n for n, _ in _programs()])
def test_blocks_reproduce_the_substituted_program(name, prog):
    B = prog.theta_blocks()
    rng = numpy.random.default_rng(0)
    ci, nb, nt = prog.cont_indices, len(prog.binary_indices), prog.num_t()
    lcp = B['lcp_rows']
    A_l, F_l = prog.A[numpy.ix_(lcp, ci)], prog.F[lcp]
    for _ in range(6):
        y = rng.integers(0, 2, nb)
        th = rng.uniform(-1.0, 1.0, nt)
        z = _z(th, y)
        S = prog.generate_substituted_problem(y.tolist(), deferred=True)
        t = th.reshape(-1, 1)
        q_S = (S.b + S.F @ t + S.A @ numpy.linalg.solve(S.Q, S.c + S.H @ t)).ravel()
        q = B['UV'] @ z
        # the substituted program scales its rows by ||[A_c | -F]||: every LCP row is one of its rows, scaled -- or, where two
        # opposite inequalities became one equality of it, that equality negated
        # (rows that differ only in their binary columns share A_c and F: one of the candidates must carry the same q)
        for i in range(len(lcp)):
            nu = numpy.linalg.norm(numpy.concatenate([A_l[i], -F_l[i]]))
            found = False
            for sign in (1.0, -1.0):
                dist = numpy.linalg.norm(S.A - sign * A_l[i] / nu, axis=1) + numpy.linalg.norm(S.F - sign * F_l[i] / nu, axis=1)
                for j in numpy.flatnonzero(dist <= 1e-12):
                    if (sign > 0 or j in S.equality_indices) and abs(q_S[j] - sign * q[i] / nu) <= 1e-9 * (1.0 + abs(q_S[j])):
                        found = True
            assert found, (name, i)
        # the objective form at random (x, y, theta)
        xc = rng.standard_normal(len(ci))
        full = numpy.zeros(prog.num_x())
        full[ci], full[prog.binary_indices] = xc, y
        form = 0.5 * xc @ B['Q_c'] @ xc + (B['G'] @ z) @ xc + 0.5 * z @ B['K'] @ z
        want = prog.evaluate_objective(full.reshape(-1, 1), t)
        assert abs(form - want) <= 1e-10 * (1.0 + abs(want)), name


def _best_kkt(Q, lin, A, rhs, n_eq, const=0.0):
    """min 1/2 x'Qx + lin'x  s.t.  A x <= rhs (first n_eq rows equalities): every active set, the feasible KKT point."""
    n, m = Q.shape[0], A.shape[0]
    best = None
    ineq = list(range(n_eq, m))
    for k in range(0, min(n - n_eq, len(ineq)) + 1):
        for extra in itertools.combinations(ineq, k):
            act = list(range(n_eq)) + list(extra)
            M = numpy.block([[Q, A[act].T], [A[act], numpy.zeros((len(act), len(act)))]])
            try:
                sol = numpy.linalg.solve(M, numpy.concatenate([-lin, rhs[act]]))
            except numpy.linalg.LinAlgError:
                continue
            x, lam = sol[:n], sol[n:]
            if numpy.any(lam[n_eq:] < -1e-9) or numpy.any(A[ineq] @ x - rhs[ineq] > 1e-9):
                continue
            val = 0.5 * x @ Q @ x + lin @ x + const
            if best is None or val < best:
                best = val
    return best


def _best_lcp(B, z):
    """The same QP from the blocks alone: every complementary basis of s = UV z + W lambda, then x = X0 z - Gt' lambda."""
    if numpy.any((B['check'] @ z)[B['check_eq'] == 0] < -1e-9) or numpy.any(numpy.abs(B['check'] @ z)[B['check_eq'] == 1] > 1e-9):
        return None
    nc, n_eq = B['n_c'], B['n_eq']
    q, W = B['UV'] @ z, B['W']
    best = None
    ineq = list(range(n_eq, nc))
    for k in range(0, len(ineq) + 1):
        for extra in itertools.combinations(ineq, k):
            act = list(range(n_eq)) + list(extra)
            lam = numpy.zeros(nc)
            if act:
                try:
                    lam[act] = numpy.linalg.solve(W[numpy.ix_(act, act)], -q[act])
                except numpy.linalg.LinAlgError:
                    continue
            s = q + W @ lam
            if numpy.any(lam[n_eq:] < -1e-9) or numpy.any(s[ineq] < -1e-9):
                continue
            x = B['X0'] @ z - B['Gt'].T @ lam
            val = 0.5 * x @ B['Q_c'] @ x + (B['G'] @ z) @ x + 0.5 * z @ B['K'] @ z
            if best is None or val < best:
                best = val
    return best


@pytest.mark.parametrize('name', ['simple_mpMIQP', 'generated'])
def test_exact_optimum_from_the_blocks_equals_the_substituted_program(name):
    prog = _golden(name) if name != 'generated' else _generated(2, 2, 6, 2, 5)
    B = prog.theta_blocks()
    rng = numpy.random.default_rng(1)
    nb, nt = len(prog.binary_indices), prog.num_t()
    compared = 0
    for y in itertools.product([0, 1], repeat=nb):
        S = prog.generate_substituted_problem(list(y), deferred=True)
        for _ in range(4):
            th = rng.uniform(-1.0, 1.0, nt) if name == 'generated' else rng.uniform(0.0, 2.0, nt)
            t = th.reshape(-1, 1)
            want = None
            if numpy.all(S.A_t @ t <= S.b_t + 1e-12):
                const = float((S.c_c + S.c_t.T @ t + 0.5 * t.T @ S.Q_t @ t)[0, 0])
                want = _best_kkt(S.Q, (S.c + S.H @ t).ravel(), S.A, (S.b + S.F @ t).ravel(), len(S.equality_indices), const)
            got = _best_lcp(B, _z(th, y))
            assert (got is None) == (want is None), (name, y, th)
            if got is not None:
                compared += 1
                assert abs(got - want) <= 1e-9 * (1.0 + abs(want)), (name, y, th)
    assert compared > 0


def test_equality_rows_that_differ_only_in_binaries_become_a_check_row():
    # x + y1 = 1 + theta  and  x + y2 = 1 + 2 theta: the same continuous row, so the second is the check row  theta + y1 - y2 = 0
    A = numpy.array([[1.0, 1.0, 0.0], [1.0, 0.0, 1.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    b = numpy.array([[1.0], [1.0], [5.0], [5.0]])
    F = numpy.array([[1.0], [2.0], [0.0], [0.0]])
    prog = _program(A, b, numpy.zeros((3, 1)), numpy.zeros((3, 1)), numpy.eye(3), numpy.array([[1.0], [-1.0]]),
                    numpy.array([[2.0], [2.0]]), F, [1, 2], equality_indices=[0, 1])
    B = prog.theta_blocks()
    assert B['n_eq'] == 1 and B['n_c'] == 3 and len(B['dependent_rows']) == 1
    assert B['check'].shape == (1, 4) and B['check_eq'].tolist() == [1]

    def accepted(theta, y):
        return abs(float(B['check'][0] @ _z([theta], y))) <= 1e-9

    assert accepted(0.0, [0, 0]) and accepted(0.0, [1, 1]) and accepted(1.0, [0, 1])
    assert not accepted(0.0, [0, 1]) and not accepted(1.0, [0, 0]) and not accepted(0.5, [0, 1])


def test_semidefinite_continuous_hessian_is_refused():
    A = numpy.array([[1.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    b = numpy.array([[2.0], [1.0], [1.0], [1.0]])
    F = numpy.array([[1.0], [0.0], [0.0], [0.0]])
    Q = numpy.diag([1.0, 0.0, 1.0])            # the second continuous variable has no curvature
    prog = _program(A, b, numpy.zeros((3, 1)), numpy.zeros((3, 1)), Q, numpy.array([[1.0], [-1.0]]), numpy.array([[1.0], [1.0]]),
                    F, [2])
    with pytest.raises(NotImplementedError):
        prog.theta_blocks()
