"""The parameter-point kernels on the MI355X against references that share none of their code (tests/theta_reference.py):
k_qp_batch (Engine.qp_solve_batch, MPQP_Program.solve_theta_batch), the MIQP kernels (_lib.miqp_solve_batch,
MPMIQP_Program.solve_theta_batch), k_lp_batch (_lib.lp_solve_batch) and MPMILP_Program.solve_theta_batch.

Programs are built with seeded numpy.  The QP shape sweeps create ``_lib.Engine`` directly, so that no presolve removes the rows
under test; the first n_eq rows are equalities.  Points whose feasibility is a knife-edge (|margin| <= 1e-7, see
theta_reference.feasibility_verdict) are counted, capped and never asserted either way."""
import numpy
import pytest

import theta_reference as tr
from ppopt_amd import MPMILP_Program, MPMIQP_Program, MPQP_Program, _lib

pytestmark = pytest.mark.gpu

KNIFE_EDGE = {'qp': 0, 'points': 0}
MAX_EDGE_FRACTION = 0.1


def _box(nt):
    return numpy.vstack([numpy.eye(nt), -numpy.eye(nt)]), numpy.ones(2 * nt)


def make_qp(seed, nc, nx, nt, n_eq, pair=True):
    """A strictly convex QP with the first n_eq rows equalities, feasible at theta = 0; with ``pair`` (and two inequality rows to
    spare) rows n_eq, n_eq + 1 are a'x <= a'x0 + 1/4 + theta_0 and -a'x <= -a'x0 + 1/4: empty for theta_0 < -1/2 whatever x."""
    rng = numpy.random.default_rng(seed)
    M = rng.standard_normal((nx, nx))
    Q = M @ M.T / nx + numpy.eye(nx)
    x0 = 0.3 * rng.standard_normal(nx)
    A = rng.standard_normal((nc, nx))
    b = A @ x0 + numpy.concatenate([numpy.zeros(n_eq), rng.uniform(0.2, 1.0, nc - n_eq)])
    F = 0.3 * rng.standard_normal((nc, nt))
    F[:n_eq] *= 0.5
    if pair and nc - n_eq >= 2:
        a = rng.standard_normal(nx)
        i = n_eq
        A[i], A[i + 1] = a, -a
        b[i], b[i + 1] = a @ x0 + 0.25, -a @ x0 + 0.25
        F[i], F[i + 1] = 0.0, 0.0
        F[i, 0] = 1.0
    c = 2.0 * rng.standard_normal(nx)
    H = rng.standard_normal((nx, nt))
    return dict(A=A, b=b, F=F, c=c, H=H, Q=Q, n_eq=n_eq)


def engine(P):
    A_t, b_t = _box(P['F'].shape[1])
    return _lib.Engine(P['A'], P['b'], P['F'], P['c'], P['H'], P['Q'], A_t, b_t, P['n_eq'])


def points(seed, nt, n_inside=24, n_facet=6, n_outside=6):
    """Inside the box, on and next to the facet theta_0 = -1/2 of the feasible set (see make_qp), outside the box."""
    rng = numpy.random.default_rng(seed + 7)
    inside = rng.uniform(-1, 1, (n_inside, nt))
    facet = rng.uniform(-1, 1, (n_facet, nt))
    facet[:, 0] = -0.5 + numpy.array([0.0, 1e-9, -1e-9, 1e-5, -1e-5, 0.0] * n_facet)[:n_facet]
    outside = rng.uniform(-1, 1, (n_outside, nt))
    outside[:, 0] = numpy.where(numpy.arange(n_outside) % 2 == 0, 1.5, -2.5)
    return numpy.vstack([inside, facet, outside])


def check_qp_points(P, th, status, x, lam, act, mp_points=1, label=''):
    """Every point against the references: status, x / lambda / objective within max(1e-9, 4e-16 cond(KKT)), the active flags.
    Returns the number of knife-edge points."""
    A, b, F, c, H, Q, n_eq = (P[k] for k in ('A', 'b', 'F', 'c', 'H', 'Q', 'n_eq'))
    edges = 0
    assert not numpy.any(status == 3), (label, 'iteration limit', numpy.flatnonzero(status == 3)[:10])
    for p in range(len(th)):
        g, r = c + H @ th[p], b + F @ th[p]
        verdict = tr.feasibility_verdict(A, r, n_eq)
        if verdict == 'edge':
            edges += 1
            continue
        if verdict == 'infeasible':
            assert status[p] == 1, (label, p, 'infeasible point reported', status[p])
            continue
        assert status[p] == 0, (label, p, 'feasible point reported', status[p], tr.feasibility_margin(A, r, n_eq))
        cert = tr.qp_certificate(Q, g, A, r, n_eq, act[p], order_hint=lam[p], use_mp=(p < mp_points and Q.shape[0] + act[p].sum() <= tr.MP_MAX_DIM) or None)
        assert cert.ok, (label, p, cert.reasons)
        tol = tr.qp_tolerance(cert)
        err = tr.compare_qp(cert, Q, g, A, x[p], lam[p], tol)
        assert err['x'] <= tol and err['lam'] <= tol and err['obj'] <= tol, (label, p, err)
        # active flags: set only on rows with zero slack; set on every row with a positive multiplier
        s = (r - A @ cert.x) / (numpy.abs(r) + numpy.abs(A) @ numpy.abs(cert.x) + 1e-300)
        assert numpy.all(numpy.abs(s[act[p]]) <= 1e-9), (label, p, 'active row with slack', numpy.abs(s[act[p]]).max())
        big = max(numpy.abs(cert.lam).max(initial=0.0), 1e-300)
        assert numpy.all(act[p][cert.lam > 1e-9 * big]), (label, p, 'row with a multiplier not flagged')
        assert numpy.all(act[p][:n_eq]), (label, p, 'equality row not flagged')
    KNIFE_EDGE['qp'] += edges
    KNIFE_EDGE['points'] += len(th)
    return edges


# ---- QP: the shape sweep --------------------------------------------------------------------------------------------------
NCS = [1, 2, 63, 64, 65, 127, 128, 129, 139]
NXS = [1, 15, 16, 17, 64, 65, 200]
NTS = [1, 8, 64]
NEQS = [0, 1, 3]


def _odd(v):
    return v if v % 2 else v + 1


def create_lds(nc, nx, nt, ne, ntc=None):
    """LDS bytes of the combinatorial kernels' layouts that mpc_create sizes for a positive definite program (the larger of its
    two layouts; mpcombi_hip.hip, make_layout); above 160 KiB mpc_create refuses the program.  ntc defaults to the box's 2 n_t."""
    ntc = 2 * nt if ntc is None else ntc
    kmax, rows_t, rows_x, nr = min(nc, nx), nc - ne + ntc, nc + ntc, nt + 1
    ld_x, ld_t = _odd(nx + nt + 3), _odd(nt + 4)
    size_K, size_L, size_X = max(kmax * kmax + kmax, kmax * nx), max(kmax * nr, 1), nx * nr

    def layout(size_T, size_E, size_X, ld_max, rows_max):
        o = sum((v + 1) & ~1 for v in (size_T, size_K, size_L, size_E, size_X))
        q = (kmax + 1) + (nc + 1) + (ld_max + 2) + 3 * (rows_max + 3) + 2 * (rows_t + 1)
        return (o * 8 + q * 4 + 15) & ~15
    return max(layout(max((rows_x + 1) * ld_x, (rows_t + 1) * ld_t), 0, 0, max(ld_x, ld_t), rows_x + 1),
               layout(max((rows_t + 2) * ld_t, rows_t * nr), rows_t * nr, size_X, ld_t, rows_t + 2))


def _shapes():
    """Every n_c with three (n_x, n_t, n_eq) in rotation; where mpc_create would refuse the program, n_t is lowered, then n_x
    (n_x = 200 fits only with n_c <= 2, n_t = 64 only with small n_c)."""
    out = []
    for k, nc in enumerate(NCS):
        for j in range(3):
            ix, nt, ne = (3 * k + j) % 7, NTS[(k + j) % 3], NEQS[(k + 2 * j) % 3]
            nx = NXS[ix]
            while create_lds(nc, nx, nt, 0) > 160 * 1024:
                if nt > 1:
                    nt = NTS[NTS.index(nt) - 1]
                else:
                    ix, nt = ix - 1, NTS[(k + j) % 3]
                    nx = NXS[ix]
            out.append((nc, nx, nt, min(ne, max(nx - 1, 0), nc)))
    out += [(1, 200, 8, 0), (2, 200, 8, 1), (2, 17, 64, 1), (139, 65, 8, 3), (65, 65, 1, 3)]
    return out


def test_sweep_covers_the_shapes():
    shapes = _shapes()
    assert all(create_lds(nc, nx, nt, ne) <= 160 * 1024 for nc, nx, nt, ne in shapes)
    for i, values in ((0, NCS), (1, NXS), (2, NTS), (3, NEQS)):
        assert set(values) <= {s[i] for s in shapes}, (i, values)
    # the refusals of mpc_create this formula predicts
    assert create_lds(63, 200, 8, 0) > 160 * 1024 and create_lds(139, 17, 64, 3) > 160 * 1024


@pytest.mark.parametrize('shape', _shapes(), ids=lambda s: 'nc%d_nx%d_nt%d_eq%d' % s)
def test_qp_shape_sweep(shape):
    nc, nx, nt, ne = shape
    seed = 1000 * nc + 10 * nx + nt + ne
    P = make_qp(seed, nc, nx, nt, ne)
    eng = engine(P)
    try:
        th = points(seed, nt)
        status, x, lam, act = eng.qp_solve_batch(th)
    finally:
        eng.close()
    edges = check_qp_points(P, th, status, x, lam, act, label=str(shape))
    assert edges <= MAX_EDGE_FRACTION * len(th) + 2, (shape, edges)


def test_qp_lds_boundary():
    """n_c = 139 is the largest tableau k_qp_batch holds in 160 KiB of LDS (solved in the sweep); 140 is refused before any launch."""
    ld = lambda nc: nc + 3 if (nc + 3) % 2 else nc + 4
    lds = lambda nc: ((nc + 1) * ld(nc) + nc) * 8 + (ld(nc) + 1 + 2 * (nc + 2) + 2) * 4 + 16
    assert lds(139) <= 160 * 1024 < lds(140)
    P = make_qp(140, 140, 16, 2, 0)
    eng = engine(P)
    try:
        with pytest.raises(_lib.MpcError, match='LDS'):
            eng.qp_solve_batch(numpy.zeros((4, 2)))
        # the handle is still usable for the rest of its work: the combinatorial root level runs
        eng.level_run(gen_children=False)
    finally:
        eng.close()


# ---- QP: degeneracy ------------------------------------------------------------------------------------------------------
def test_qp_duplicate_and_parallel_rows():
    P = make_qp(21, 24, 8, 3, 1)
    k = [1, 2, 5, 9]
    P['A'] = numpy.vstack([P['A'], P['A'][k], 2.0 * P['A'][k]])
    P['b'] = numpy.concatenate([P['b'], P['b'][k], 2.0 * P['b'][k]])
    P['F'] = numpy.vstack([P['F'], P['F'][k], 2.0 * P['F'][k]])
    eng = engine(P)
    try:
        th = points(21, 3, n_inside=60)
        status, x, lam, act = eng.qp_solve_batch(th)
    finally:
        eng.close()
    check_qp_points(P, th, status, x, lam, act, mp_points=3, label='duplicates')


def _vertex_program(seed, nx, n_rows, n_strong):
    """n_rows rows through x* = 1 at theta = 0 (all weakly or strongly active there), n_strong of them with multipliers
    in [1, 2], the rest weakly active (multiplier zero) -- n_rows >= n_x rows meet at one point."""
    rng = numpy.random.default_rng(seed)
    xs = numpy.ones(nx)
    A = rng.standard_normal((n_rows, nx))
    b = A @ xs
    M = rng.standard_normal((nx, nx))
    Q = M @ M.T + numpy.eye(nx)
    lam = numpy.zeros(n_rows)
    lam[:n_strong] = rng.uniform(1.0, 2.0, n_strong)
    c = -Q @ xs - A.T @ lam
    F = numpy.zeros((n_rows, 2))
    F[:, 0] = 0.1 * rng.standard_normal(n_rows)
    H = numpy.zeros((nx, 2))
    H[:, 1] = rng.standard_normal(nx)
    return dict(A=A, b=b, F=F, c=c, H=H, Q=Q, n_eq=0), xs, lam


@pytest.mark.parametrize('nx,n_rows,n_strong', [(4, 8, 2), (6, 6, 0), (5, 12, 5), (16, 70, 3)])
def test_qp_many_weakly_active_rows(nx, n_rows, n_strong):
    P, xs, lam0 = _vertex_program(nx * 100 + n_rows, nx, n_rows, n_strong)
    th = numpy.vstack([numpy.zeros((1, 2)), numpy.random.default_rng(3).uniform(-1, 1, (20, 2)) * numpy.array([1e-3, 1.0]),
                       [[0.0, 1e-9], [0.0, -1e-9]]])
    eng = engine(P)
    try:
        status, x, lam, act = eng.qp_solve_batch(th)
    finally:
        eng.close()
    assert status[0] == 0 and numpy.max(numpy.abs(x[0] - xs)) <= 1e-9 * nx
    # with more active rows than n_x the multipliers are not unique: any lambda >= 0 with A'lambda = A'lambda0 is one
    assert numpy.max(numpy.abs(P['A'].T @ (lam[0] - lam0))) <= 1e-8 * max(1.0, lam0.max()) * n_rows
    assert lam[0].min() >= -1e-12 * max(1.0, lam0.max())
    check_qp_points(P, th, status, x, lam, act, mp_points=2, label='weakly active')


def test_qp_exact_ties_in_q():
    """Q = I, rows e_i with equal right-hand sides, c = -5 (1, .., 1): every q_i is the same number, the start row is a tie."""
    nx, nt = 8, 2
    A = numpy.vstack([numpy.eye(nx), -numpy.eye(nx)])
    b = numpy.ones(2 * nx)
    F = numpy.zeros((2 * nx, nt))
    F[:nx, 0] = 1.0
    P = dict(A=A, b=b, F=F, c=-5.0 * numpy.ones(nx), H=numpy.zeros((nx, nt)), Q=numpy.eye(nx), n_eq=0)
    th = numpy.array([[0.0, 0.0], [0.5, 0.0], [-0.5, 1.0], [0.25, -1.0]])
    eng = engine(P)
    try:
        status, x, lam, act = eng.qp_solve_batch(th)
    finally:
        eng.close()
    assert numpy.all(status == 0)
    for p in range(len(th)):
        assert numpy.array_equal(x[p], numpy.full(nx, 1.0 + th[p, 0])), (p, x[p])
        assert numpy.allclose(lam[p][:nx], 4.0 - th[p, 0], rtol=1e-14) and not lam[p][nx:].any()
    check_qp_points(P, th, status, x, lam, act, mp_points=4, label='ties')


# ---- QP: scaling ---------------------------------------------------------------------------------------------------------
def _solve(P, th):
    eng = engine(P)
    try:
        return eng.qp_solve_batch(th)
    finally:
        eng.close()


SCALE_TH = numpy.random.default_rng(5).uniform(-1, 1, (40, 3))


@pytest.mark.parametrize('s', [1e-6, 1e6, 1e10])
def test_qp_hessian_scaling(s):
    """Q, c, H scaled by s: the same minimiser, multipliers scaled by s.  (s = 1e10 puts every entry of W = A Q^-1 A' below
    the pivot tolerance of an unscaled tableau.)"""
    P0 = make_qp(31, 20, 6, 3, 1)
    P = dict(P0, Q=s * P0['Q'], c=s * P0['c'], H=s * P0['H'])
    st0, x0, l0, a0 = _solve(P0, SCALE_TH)
    st, x, lam, act = _solve(P, SCALE_TH)
    check_qp_points(P0, SCALE_TH, st0, x0, l0, a0, label='s=1')
    check_qp_points(P, SCALE_TH, st, x, lam, act, mp_points=2, label=f's={s}')
    assert numpy.array_equal(st, st0)
    ok = st == 0
    assert numpy.max(numpy.abs(x[ok] - x0[ok])) <= 1e-9 * numpy.abs(x0[ok]).max()
    assert numpy.max(numpy.abs(lam[ok] / s - l0[ok])) <= 1e-9 * numpy.abs(l0[ok]).max()


@pytest.mark.parametrize('which', ['rows', 'equalities'])
def test_qp_row_scaling(which):
    """Rows scaled by 1e6 / 1e-6 (alternately), or the equality rows by 1e-7: the same minimiser, multipliers divided by the row scale."""
    P0 = make_qp(41, 20, 6, 3, 3)
    d = numpy.ones(20)
    if which == 'rows':
        d[3:] = numpy.where(numpy.arange(17) % 2 == 0, 1e6, 1e-6)
    else:
        d[:3] = 1e-7
    P = dict(P0, A=d[:, None] * P0['A'], b=d * P0['b'], F=d[:, None] * P0['F'])
    st0, x0, l0, _ = _solve(P0, SCALE_TH)
    st, x, lam, act = _solve(P, SCALE_TH)
    check_qp_points(P, SCALE_TH, st, x, lam, act, mp_points=2, label=which)
    assert numpy.array_equal(st, st0)
    ok = st == 0
    assert numpy.max(numpy.abs(x[ok] - x0[ok])) <= 1e-9 * numpy.abs(x0[ok]).max()
    assert numpy.max(numpy.abs(lam[ok] * d - l0[ok])) <= 1e-9 * numpy.abs(l0[ok]).max()


def test_qp_ill_conditioned_hessian():
    rng = numpy.random.default_rng(51)
    P = make_qp(51, 16, 8, 2, 1)
    U = numpy.linalg.qr(rng.standard_normal((8, 8)))[0]
    P['Q'] = U @ numpy.diag(numpy.logspace(0, 8, 8)) @ U.T
    P['Q'] = 0.5 * (P['Q'] + P['Q'].T)
    th = points(51, 2)
    st, x, lam, act = _solve(P, th)
    check_qp_points(P, th, st, x, lam, act, mp_points=3, label='kappa 1e8')


def test_qp_dependent_consistent_equalities():
    """Equality row 2 = row 0 + row 1 (right-hand sides and theta columns summed): consistent everywhere.  mpc_create may refuse
    the program; if it takes it, every point is solved."""
    P = make_qp(61, 12, 5, 2, 3)
    for k in ('A', 'b', 'F'):
        P[k][2] = P[k][0] + P[k][1]
    try:
        eng = engine(P)
    except _lib.MpcError:
        return
    try:
        th = points(61, 2)
        status, x, lam, act = eng.qp_solve_batch(th)
    finally:
        eng.close()
    check_qp_points(P, th, status, x, lam, act, mp_points=2, label='dependent equalities')
    # the dependent row carries no multiplier of its own, the solution is that of the program without it
    Q = dict(P, A=numpy.delete(P['A'], 2, 0), b=numpy.delete(P['b'], 2), F=numpy.delete(P['F'], 2, 0), n_eq=2)
    st2, x2, _, _ = _solve(Q, th)
    assert numpy.array_equal(status, st2)
    ok = status == 0
    assert numpy.max(numpy.abs(x[ok] - x2[ok])) <= 1e-9 * numpy.abs(x2[ok]).max()


# ---- QP: batch mechanics -------------------------------------------------------------------------------------------------
def _same(a, b):
    """Bit for bit (NaN payloads included: x is NaN at infeasible points)."""
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_qp_batch_mechanics():
    import torch
    P = make_qp(71, 20, 10, 3, 2)
    Pb = make_qp(72, 30, 12, 3, 0)
    nc = 20
    ld = nc + 3 if (nc + 3) % 2 else nc + 4
    lds = ((nc + 1) * ld + nc) * 8 + (ld + 1 + 2 * (nc + 2) + 2) * 4 + 16
    grid = torch.cuda.get_device_properties(0).multi_processor_count * max(1, min(16, 160 * 1024 // lds))
    rng = numpy.random.default_rng(73)
    big = rng.uniform(-1, 1, (200000, 3))
    e1, e2 = engine(P), engine(Pb)
    try:
        full = e1.qp_solve_batch(big)
        check_qp_points(P, big[:300], *(a[:300] for a in full), label='m=2e5')
        assert (full[0] == 1).sum() > 1000 and (full[0] == 0).sum() > 1000
        for m in (1, 2, grid - 1, grid, grid + 1):
            part = e1.qp_solve_batch(big[:m])
            for a, b in zip(part, full):
                assert _same(a, b[:m]), m
        for p in rng.choice(200000, 40, replace=False):
            one = e1.qp_solve_batch(big[p:p + 1])
            for a, b in zip(one, full):
                assert _same(a[0], b[p]), p
        perm = rng.permutation(grid + 1)
        pr = e1.qp_solve_batch(big[perm])
        for a, b in zip(pr, full):
            assert _same(a, b[perm])
        # two handles used alternately
        o2 = e2.qp_solve_batch(big[:5000])
        again1 = e1.qp_solve_batch(big[:5000])
        again2 = e2.qp_solve_batch(big[:5000])
        for a, b, c, d in zip(again1, full, again2, o2):
            assert _same(a, b[:5000]) and _same(c, d)
    finally:
        e1.close()
        e2.close()


def test_mpqp_program_solve_theta_batch():
    """The public API on a program with presolve: every answer against the certificate of its own active set."""
    P = make_qp(81, 14, 5, 2, 0)
    A_t, b_t = _box(2)
    prog = MPQP_Program(P['A'], P['b'].reshape(-1, 1), P['c'].reshape(-1, 1), P['H'], P['Q'], A_t, b_t.reshape(-1, 1), P['F'])
    th = numpy.random.default_rng(82).uniform(-1, 1, (60, 2))
    res = prog.solve_theta_batch(th)
    ne = len(prog.equality_indices)
    assert list(prog.equality_indices) == list(range(ne))
    for p, r in enumerate(res):
        g, rr = (prog.c + prog.H @ th[p].reshape(-1, 1)).ravel(), (prog.b + prog.F @ th[p].reshape(-1, 1)).ravel()
        v = tr.feasibility_verdict(prog.A, rr, ne)
        if v == 'edge':
            continue
        assert (r is not None) == (v == 'feasible'), p
        if r is None:
            continue
        act = numpy.zeros(len(rr), dtype=bool)
        act[r.active_set] = True
        cert = tr.qp_certificate(prog.Q, g, prog.A, rr, ne, act, order_hint=r.dual)
        assert cert.ok, (p, cert.reasons)
        assert abs(r.obj - cert.obj) <= tr.qp_tolerance(cert) * max(1.0, abs(cert.obj))


# ---- MIQP -----------------------------------------------------------------------------------------------------------------
def make_miqp(seed, nxc, nb, nc, n_eq=0, check_eq=False):
    """Continuous variables first, then nb binaries.  Rows mix both; with ``check_eq`` two equality rows differ only in their
    binary columns (one becomes a check row)."""
    rng = numpy.random.default_rng(seed)
    nx, nt = nxc + nb, 2
    M = rng.standard_normal((nx, nx))
    Q = M @ M.T / nx + numpy.eye(nx)
    A = rng.standard_normal((nc, nx))
    b = rng.uniform(0.5, 2.0, nc) + numpy.abs(A[:, nxc:]).sum(axis=1)
    F = 0.3 * rng.standard_normal((nc, nt))
    if n_eq:
        b[:n_eq] = 0.1 * rng.standard_normal(n_eq)
    if check_eq:
        A[1, :nxc] = A[0, :nxc]
        A[1, nxc:] = A[0, nxc:] + 1.0
        b[1] = b[0] + 1.0
        F[1] = F[0]                        # the check row 1 - sum(y) = 0: one binary set
    c = rng.standard_normal(nx)
    H = 0.5 * rng.standard_normal((nx, nt))
    A_t, b_t = _box(nt)
    prog = MPMIQP_Program(A, b.reshape(-1, 1), c.reshape(-1, 1), H, Q, A_t, b_t.reshape(-1, 1), F, list(range(nxc, nx)),
                          equality_indices=list(range(n_eq)) if n_eq else None)
    return prog


def _first_eq(prog):
    """The program's rows with its equality rows first (theta_reference's convention) and their count."""
    eq = list(prog.equality_indices)
    order = eq + [i for i in range(prog.A.shape[0]) if i not in eq]
    return prog.A[order], prog.b[order].ravel(), prog.F[order], len(eq)


def check_miqp(prog, th, leaves=None, label=''):
    A, b, F, ne = _first_eq(prog)
    Y = numpy.asarray(prog.feasible_combinations() if leaves is None else leaves, dtype=numpy.float64)
    B = prog.theta_blocks()
    status, leaf, obj, x, lam, act = _lib.miqp_solve_batch(B, Y, th)
    res = prog.solve_theta_batch(th, leaves=None if leaves is None else leaves)
    assert not numpy.any(status == 3), label
    n_opt = 0
    for p in range(len(th)):
        best, objs = tr.miqp_brute_force(prog.Q, prog.c.ravel(), prog.H, A, b, F, ne, prog.binary_indices, Y, th[p])
        const = float(prog.c_c[0, 0] + prog.c_t.ravel() @ th[p] + 0.5 * th[p] @ prog.Q_t @ th[p])
        if best is None:
            assert status[p] == 1 and leaf[p] == -1 and res[p] is None, (label, p)
            continue
        n_opt += 1
        assert status[p] == 0, (label, p, status[p], best)
        assert abs(obj[p] - (best + const)) <= 1e-9 * max(1.0, abs(best)), (label, p, obj[p], best)
        assert objs[leaf[p]] is not None and abs(objs[leaf[p]] - best) <= 1e-9 * max(1.0, abs(best)), (label, p)
        assert res[p] is not None and res[p].obj == obj[p]
    return n_opt


@pytest.mark.parametrize('nxc,nb,nc,n_eq,check_eq', [(3, 1, 6, 0, False), (1, 3, 5, 0, False), (4, 5, 8, 1, False),
                                                     (3, 4, 7, 2, True), (5, 8, 9, 0, False), (2, 2, 4, 0, True)])
def test_miqp_against_brute_force(nxc, nb, nc, n_eq, check_eq):
    prog = make_miqp(nxc * 1000 + nb * 100 + nc, nxc, nb, nc, n_eq, check_eq)
    th = numpy.random.default_rng(nc).uniform(-1, 1, (12, 2))
    n_opt = check_miqp(prog, th, label=f'{nxc},{nb},{nc}')
    assert n_opt >= 6


def test_miqp_without_lcp_rows():
    """n_c = 0: no row has continuous content (pure-binary rows and check rows only); the continuous part is unconstrained."""
    rng = numpy.random.default_rng(91)
    nxc, nb, nt = 3, 3, 2
    nx = nxc + nb
    M = rng.standard_normal((nx, nx))
    Q = M @ M.T / nx + numpy.eye(nx)
    A = numpy.zeros((4, nx))
    A[0, nxc:] = [1.0, 1.0, 0.0]           # pure binary: y0 + y1 <= 1
    A[1, nxc:] = [0.0, 1.0, 1.0]           # check row: y1 + y2 <= 1 + theta_0
    A[2, nxc:] = [-1.0, 0.0, 0.0]          # check row: -y0 <= -0.5 + theta_1  (y0 = 1 unless theta_1 >= 0.5)
    A[3, nxc:] = [0.0, 0.0, 1.0]           # pure binary: y2 <= 1
    b = numpy.array([1.0, 1.0, -0.5, 1.0])
    F = numpy.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])
    A_t, b_t = _box(nt)
    prog = MPMIQP_Program(A, b.reshape(-1, 1), rng.standard_normal((nx, 1)), rng.standard_normal((nx, nt)), Q, A_t,
                          b_t.reshape(-1, 1), F, list(range(nxc, nx)))
    B = prog.theta_blocks()
    assert int(B['n_c']) == 0
    th = numpy.vstack([numpy.random.default_rng(92).uniform(-1, 1, (10, 2)), [[-1.0, 0.75], [0.5, 0.0]]])
    assert check_miqp(prog, th, label='n_c = 0') >= 6


def test_miqp_exact_ties_go_to_the_lowest_leaf():
    """Duplicated fixations and a binary that appears nowhere: fixations differing only there tie bit for bit; the lowest index wins."""
    rng = numpy.random.default_rng(101)
    nxc, nb, nt = 3, 3, 2
    nx = nxc + nb
    M = rng.standard_normal((nxc, nxc))
    Q = numpy.eye(nx)
    Q[:nxc, :nxc] = M @ M.T / nxc + numpy.eye(nxc)
    A = rng.standard_normal((6, nx))
    A[:, nx - 1] = 0.0                     # binary 2 appears nowhere: no row, no objective term
    b = rng.uniform(1.0, 2.0, 6) + numpy.abs(A[:, nxc:]).sum(axis=1)
    F = 0.3 * rng.standard_normal((6, nt))
    c = rng.standard_normal(nx)
    c[nx - 1] = 0.0
    H = rng.standard_normal((nx, nt))
    H[nx - 1] = 0.0
    Q[nx - 1, nx - 1] = 0.0
    A_t, b_t = _box(nt)
    prog = MPMIQP_Program(A, b.reshape(-1, 1), c.reshape(-1, 1), H, Q, A_t, b_t.reshape(-1, 1), F, list(range(nxc, nx)))
    leaves = [[1, 0, 1], [0, 1, 0], [1, 0, 0], [0, 1, 1], [0, 1, 0], [1, 1, 0], [1, 1, 1], [0, 0, 1], [0, 0, 0]]
    th = numpy.random.default_rng(102).uniform(-1, 1, (30, 2))
    B = prog.theta_blocks()
    Y = numpy.asarray(leaves, dtype=numpy.float64)
    status, leaf, obj, x, lam, act = _lib.miqp_solve_batch(B, Y, th)
    # each leaf alone: the objective of every (point, leaf) pair
    per = numpy.stack([_lib.miqp_solve_batch(B, Y[l:l + 1], th)[2] for l in range(len(Y))], axis=1)
    for p in range(len(th)):
        ok = numpy.isfinite(per[p])
        assert status[p] == 0 and ok.any()
        want = int(numpy.flatnonzero(per[p] == per[p][ok].min())[0])
        assert leaf[p] == want, (p, leaf[p], want, per[p])
        assert obj[p] == per[p][want]
        twins = [l for l in range(len(Y)) if numpy.array_equal(Y[l, :2], Y[want, :2])]
        assert all(per[p][l] == per[p][want] for l in twins), (p, per[p])   # the binary that appears nowhere: exact ties
        assert leaf[p] == min(twins)
    check_miqp(prog, th[:8], leaves=leaves, label='ties')


def test_miqp_every_leaf_infeasible():
    prog = make_miqp(111, 2, 2, 5)
    A, b, F = prog.A.copy(), prog.b.copy(), prog.F.copy()
    # x_0 <= 1 + theta_0 and -x_0 <= 1 + theta_0: empty for theta_0 < -1, whatever the binaries
    row = numpy.zeros((2, A.shape[1]))
    row[0, 0], row[1, 0] = 1.0, -1.0
    Fr = numpy.zeros((2, F.shape[1]))
    Fr[:, 0] = 1.0
    A_t, b_t = _box(2)
    prog = MPMIQP_Program(numpy.vstack([A, row]), numpy.vstack([b, [[1.0], [1.0]]]), prog.c, prog.H, prog.Q, A_t, b_t.reshape(-1, 1),
                          numpy.vstack([F, Fr]), prog.binary_indices)
    B = prog.theta_blocks()
    Y = numpy.asarray(prog.feasible_combinations(), dtype=numpy.float64)
    th = numpy.array([[-3.0, 0.0], [-1.5, 0.5], [0.0, 0.0]])
    status, leaf, obj, x, lam, act = _lib.miqp_solve_batch(B, Y, th)
    for p in (0, 1):
        assert status[p] == 1 and leaf[p] == -1 and numpy.isnan(obj[p])
        assert numpy.all(numpy.isnan(x[p])) and not lam[p].any() and not act[p].any()
    assert status[2] == 0 and leaf[2] >= 0
    assert prog.solve_theta_batch(th)[:2] == [None, None]


# ---- LP / MILP -------------------------------------------------------------------------------------------------------------
def _lp_lds(m, n):
    ld = n + 3 if (n + 3) % 2 else n + 4
    return (((m + 1) * ld * 8 + (ld + 1 + 3 * (m + 2)) * 4) + 15) & ~15


def _lp_m_max(n):
    m = 1
    while _lp_lds(m + 1, n) <= 160 * 1024:
        m += 1
    return m


def _random_lps(rng, k, m, n, bounded=True):
    """k LPs [m, n]: feasible (x0 strictly inside), bounded when c = -A' y with y >= 0 on n + 1 rows."""
    A = rng.standard_normal((k, m, n))
    x0 = rng.standard_normal((k, n))
    b = numpy.einsum('kmn,kn->km', A, x0) + rng.uniform(0.1, 1.0, (k, m))
    y = numpy.zeros((k, m))
    for i in range(k):
        y[i, rng.choice(m, min(m, n + 1), replace=False)] = rng.uniform(0.5, 1.5, min(m, n + 1))
    c = -numpy.einsum('kmn,km->kn', A, y) if bounded else rng.standard_normal((k, n))
    return A, b, c, x0


def _check_lps(A, b, c, eq, label, tol=1e-9):
    st, x, obj, _ = _lib.lp_solve_batch(A, b, c, eq)
    assert not numpy.any(st == 3), label
    for i in range(len(st)):
        rs, rf = tr.lp_reference(A[i], b[i], c[i], eq[i])
        assert st[i] == rs, (label, i, st[i], rs)
        if rs == 0:
            assert abs(obj[i] - rf) <= tol * max(1.0, abs(rf)), (label, i, obj[i], rf)
            viol = (A[i] @ x[i] - b[i]) / (numpy.abs(b[i]) + numpy.abs(A[i]) @ numpy.abs(x[i]))
            assert viol.max() <= 1e-9 and numpy.all(numpy.abs(viol[eq[i]]) <= 1e-9), (label, i)
    return st


@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_lp_shape_edges(n):
    rng = numpy.random.default_rng(n)
    m_max = _lp_m_max(n)
    for m in sorted({max(1, n // 2), n, n + 1, 2 * n + 3, min(m_max, 200), m_max}):
        k = 3 if m > 1000 else 6
        A, b, c, x0 = _random_lps(rng, k, m, n)
        eq = numpy.zeros((k, m), dtype=bool)
        if m > n + 1:
            # row 0 an equality through x0's neighbourhood: a0'x = a0'x0 + 0.05 (x0 keeps a slack of at least 0.1 elsewhere)
            eq[:, 0] = True
            b[:, 0] = numpy.einsum('kn,kn->k', A[:, 0], x0) + 0.05 * numpy.linalg.norm(A[:, 0], axis=1) / numpy.sqrt(n + 1)
        _check_lps(A, b, c, eq, f'n={n} m={m}')
    A, b, c, _ = _random_lps(rng, 1, m_max + 1, n)
    with pytest.raises(_lib.MpcError, match='LDS'):
        _lib.lp_solve_batch(A, b, c, numpy.zeros((1, m_max + 1), dtype=bool))


def test_lp_degenerate_unbounded_and_scaled():
    rng = numpy.random.default_rng(121)
    m, n, k = 30, 6, 8
    A, b, c, _ = _random_lps(rng, k, m, n)
    # degenerate: rows 20.. pass through a common vertex of rows 0..5, duplicates of rows 6..9
    for i in range(k):
        v = numpy.linalg.solve(A[i, :n], b[i, :n])
        A[i, 20:26] = rng.standard_normal((6, n))
        b[i, 20:26] = A[i, 20:26] @ v
        A[i, 26:30] = A[i, 6:10]
        b[i, 26:30] = b[i, 6:10]
    eq = numpy.zeros((k, m), dtype=bool)
    _check_lps(A, b, c, eq, 'degenerate')
    # unbounded: a random cost on a cone-shaped feasible set (the first n + 1 rows dropped to open it)
    Au, bu, cu, _ = _random_lps(rng, k, 4, n, bounded=False)
    st = _check_lps(Au, bu, cu, numpy.zeros((k, 4), dtype=bool), 'unbounded')
    assert numpy.any(st == 2)
    # rows scaled by 1e6 / 1e-6: the same optimum
    d = numpy.where(numpy.arange(m) % 2 == 0, 1e6, 1e-6)
    A2, b2, c2, _ = _random_lps(rng, k, m, n)
    st0, _, f0, _ = _lib.lp_solve_batch(A2, b2, c2, eq)
    st1 = _check_lps(d[None, :, None] * A2, d[None, :] * b2, c2, eq, 'scaled rows', tol=1e-8)
    assert numpy.array_equal(st0, st1)


def test_milp_against_highs():
    rng = numpy.random.default_rng(131)
    for seed in range(4):
        nxc, nb, nt, nc = 3, 3, 2, 8
        nx = nxc + nb
        A = rng.standard_normal((nc, nx))
        b = rng.uniform(0.5, 2.0, nc) + numpy.abs(A[:, nxc:]).sum(axis=1)
        box = numpy.hstack([numpy.vstack([numpy.eye(nxc), -numpy.eye(nxc)]), numpy.zeros((2 * nxc, nb))])
        A = numpy.vstack([A, box])
        b = numpy.concatenate([b, 3.0 * numpy.ones(2 * nxc)])
        F = numpy.vstack([0.3 * rng.standard_normal((nc, nt)), numpy.zeros((2 * nxc, nt))])
        c = rng.standard_normal(nx)
        H = rng.standard_normal((nx, nt))
        A_t, b_t = _box(nt)
        prog = MPMILP_Program(A, b.reshape(-1, 1), c.reshape(-1, 1), H, A_t, b_t.reshape(-1, 1), F, list(range(nxc, nx)))
        th = rng.uniform(-1, 1, (15, nt))
        res = prog.solve_theta_batch(th)
        eqm = numpy.zeros(prog.A.shape[0], dtype=bool)
        eqm[list(prog.equality_indices)] = True
        for p in range(len(th)):
            t = th[p].reshape(-1, 1)
            st, f = tr.milp_reference(prog.A, (prog.b + prog.F @ t).ravel(), (prog.c + prog.H @ t).ravel(), eqm, prog.binary_indices)
            const = float(prog.c_c[0, 0] + prog.c_t.ravel() @ th[p] + 0.5 * th[p] @ prog.Q_t @ th[p])
            assert (res[p] is not None) == (st == 0), (seed, p)
            if st == 0:
                assert abs(res[p].obj - (f + const)) <= 1e-9 * max(1.0, abs(f)), (seed, p, res[p].obj, f)


# ---- the stateless calls from several threads ---------------------------------------------------------------------------------
def test_stateless_point_calls_from_four_threads():
    """lp_solve_batch, miqp_solve_batch and facet_centres hold no handle: each call has buffers of its own, and the first two a
    stream of their own.  Four threads make the three calls eight times each, all at once; every array of every call is bit for
    bit what the same call returned serially beforehand."""
    import threading
    rng = numpy.random.default_rng(141)
    A, b, c, _ = _random_lps(rng, 64, 30, 6)
    eq = numpy.zeros((64, 30), dtype=bool)
    prog = make_miqp(3 * 1000 + 1 * 100 + 6, 3, 1, 6)   # the first (and smallest) case of test_miqp_against_brute_force
    B, Y = prog.theta_blocks(), numpy.asarray(prog.feasible_combinations(), dtype=numpy.float64)
    th = rng.uniform(-1, 1, (50, 2))
    # n_theta = 2: three boxes |theta_i - o_i| <= r and two simplices theta >= o, sum(theta - o) <= r, rows [f | E]
    E_box, E_sim = numpy.vstack([numpy.eye(2), -numpy.eye(2)]), numpy.vstack([-numpy.eye(2), numpy.ones((1, 2))])
    polys = []
    for k in range(5):
        o, r = rng.uniform(-1, 1, 2), rng.uniform(0.5, 2.0)
        E = E_box if k % 2 == 0 else E_sim
        f = E @ o + (r if k % 2 == 0 else numpy.array([0.0, 0.0, r]))
        polys.append(numpy.hstack([f.reshape(-1, 1), E]))
    ef, row_off = numpy.vstack(polys), numpy.cumsum([0] + [len(p) for p in polys])
    calls = [lambda: _lib.lp_solve_batch(A, b, c, eq), lambda: _lib.miqp_solve_batch(B, Y, th), lambda: _lib.facet_centres(ef, row_off)]
    want = [f() for f in calls]
    assert numpy.all(want[0][0] == 0) and numpy.any(want[1][0] == 0) and numpy.all(want[2][2] == 0) and numpy.all(want[2][1] > 0)
    bad, start = [], threading.Barrier(4)

    def worker(t):
        try:
            start.wait()
            for r in range(8):
                for k, f in enumerate(calls):
                    got = f()
                    if len(got) != len(want[k]) or not all(_same(g, w) for g, w in zip(got, want[k])):
                        bad.append((t, r, k))
        except Exception as e:   # an MpcError of a call: reported by the main thread
            bad.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, bad


def test_knife_edge_count_is_small():
    """Runs last in this module: the knife-edge points excluded across the QP tests, capped."""
    if KNIFE_EDGE['points']:
        assert KNIFE_EDGE['qp'] <= MAX_EDGE_FRACTION * KNIFE_EDGE['points'], KNIFE_EDGE
    print(f"knife-edge QP points excluded: {KNIFE_EDGE['qp']} of {KNIFE_EDGE['points']}")
