"""Host reference for closed-loop simulation (Solution.simulate): a plain loop over Solution.get_region and
CriticalRegion.evaluate, the way the reference's MPC tutorial steps an explicit controller.  No device, no code of ppopt_amd.closed_loop.
A plain helper module (not a conftest), imported by tests/test_closed_loop_cpu.py and tests/test_gpu_closed_loop.py."""
import math

import numpy

import locate_reference as lref


def simulate(solution, theta0, steps, A, B, inputs, c=None, w=None, stop_tol=None):
    """One trajectory per row of theta0.  Returns a dict of theta [n, steps+1, n_t], u [n, steps, n_u], region [n, steps] (the index in
    critical_regions), status [n] (0 ran, 1 steady, 2 no region, 3 non-finite) and exit_step [n]; NaN / -1 after a trajectory's end.
    theta_{k+1,i} = c_i + sum_j A_ij theta_j + sum_l B_il u_l + w_i, summed in this order."""
    theta0 = numpy.atleast_2d(numpy.asarray(theta0, dtype=float))
    A = numpy.asarray(A, dtype=float)
    B = numpy.asarray(B, dtype=float).reshape(len(A), -1)
    n, nt = theta0.shape
    nu = B.shape[1]
    index = {id(cr): j for j, cr in enumerate(solution.critical_regions)}
    out = {'theta': numpy.full((n, steps + 1, nt), numpy.nan), 'u': numpy.full((n, steps, nu), numpy.nan),
           'region': numpy.full((n, steps), -1, dtype=numpy.int64), 'status': numpy.zeros(n, dtype=numpy.int32),
           'exit_step': numpy.full(n, steps, dtype=numpy.int32)}
    for p in range(n):
        th = theta0[p].copy()
        out['theta'][p, 0] = th
        for k in range(steps):
            if not numpy.all(numpy.isfinite(th)):
                out['status'][p], out['exit_step'][p] = 3, k
                break
            cr = solution.get_region(th.reshape(-1, 1))
            if cr is None:
                out['status'][p], out['exit_step'][p] = 2, k
                break
            x = numpy.asarray(cr.evaluate(th.reshape(-1, 1)), dtype=float).reshape(-1)
            u = x[list(inputs)]
            nxt = numpy.empty(nt)
            for i in range(nt):
                v = 0.0 if c is None else float(c[i])
                for j in range(nt):
                    v = v + A[i, j] * th[j]
                for l in range(nu):
                    v = v + B[i, l] * u[l]
                if w is not None:
                    v = v + w[p, k, i]
                nxt[i] = v
            out['region'][p, k] = index[id(cr)]
            out['u'][p, k] = u
            out['theta'][p, k + 1] = nxt
            steady = stop_tol is not None and bool(numpy.all(numpy.abs(nxt - th) <= stop_tol))
            th = nxt
            if steady:
                out['status'][p], out['exit_step'][p] = 1, k + 1
                break
    return out


# ---- the contract on stacked rows, in exact arithmetic -----------------------------------------------------------------------------
# mpc_locator_simulate (include/mpcombi.h) restated for data on a dyadic lattice.  Every number is held as a Python int times a power of
# two, so nothing is rounded; every u, every theta and every difference the device forms is asserted to be a float64, and with it
# every partial sum of its terms in any order: a sum of multiples of 2^e whose absolute values add up to less than 2^(e + 53) is a
# float64 at every stage, fused or not.  The device then has one admissible answer, and a test compares bit patterns.
def _ints(a):
    """(I, e): a == I 2^e exactly, I an object array of Python ints of a's shape, e <= 0 the finest exponent of any entry"""
    a = numpy.asarray(a, dtype=float)
    pairs = [float(v).as_integer_ratio() for v in a.ravel()]
    d = max([den.bit_length() - 1 for _, den in pairs], default=0)
    out = numpy.empty(a.size, dtype=object)
    for i, (num, den) in enumerate(pairs):
        out[i] = num << (d - (den.bit_length() - 1))
    return out.reshape(a.shape), -d


def _floats(I, e, mag=None):
    """(the float64 array equal to I 2^e, bits): asserts that every entry is a float64; bits = the widest sum of absolute terms `mag`
    (default |I|) in units of 2^e, which bounds every partial sum"""
    out = numpy.empty(I.shape)
    bits = 0
    flat, fm = I.ravel(), (I if mag is None else mag).ravel()
    for i in range(flat.size):
        v, m = int(flat[i]), int(fm[i])
        assert abs(v) <= m
        bits = max(bits, m.bit_length())
        assert m.bit_length() <= 53 and e >= -1022 and e + m.bit_length() <= 1023, (v, m, e)
        out.ravel()[i] = math.ldexp(v, e)
    return out, bits


def _absI(I):
    return numpy.vectorize(abs, otypes=[object])(I) if I.size else I


def simulate_rows(row_off, ef, xlaw, theta0, steps, A, B, inputs, c=None, w=None, tol=0.0, stop_tol=None, overlapping=False,
                  inclusive=False, Q=None, cvec=None, H=None):
    """The closed loop over stacked rows [f | E] and laws [b | A] (the arrays of mpc_locator_create), one trajectory per row of theta0;
    w [n, steps, n_t].  Per step: status 3 for a non-finite state; the region by locate_reference.locate, status 2 when there is none;
    u = the rows `inputs` of the region's law at theta; theta+ = c + A theta + B u + w; status 1 when |theta+ - theta|_inf <= stop_tol.
    Returns the dict of `simulate` (NaN / -1 after a trajectory's end) with 'traj_steps' (steps taken over all trajectories; the step
    that finds no region counts) and 'bits' (the widest sum met, row tests and objective included: the exactness certificate is
    bits <= 53, and it is asserted on the way)."""
    theta0 = numpy.atleast_2d(numpy.asarray(theta0, dtype=float))
    n, nt = theta0.shape
    A = numpy.asarray(A, dtype=float).reshape(nt, nt)
    B = numpy.asarray(B, dtype=float).reshape(nt, -1)
    inputs = [int(i) for i in inputs]
    nu = len(inputs)
    assert B.shape[1] == nu
    ef, xlaw = numpy.asarray(ef, dtype=float), numpy.asarray(xlaw, dtype=float)
    LI, eL = _ints(xlaw[:, inputs, :])
    AI, eA = _ints(A)
    BI, eB = _ints(B)
    cI, ec = _ints(numpy.zeros(nt) if c is None else numpy.asarray(c, dtype=float).reshape(nt))
    wI, ew = _ints(numpy.zeros((n, steps, nt)) if w is None else numpy.asarray(w, dtype=float).reshape(n, steps, nt))
    out = {'theta': numpy.full((n, steps + 1, nt), numpy.nan), 'u': numpy.full((n, steps, nu), numpy.nan),
           'region': numpy.full((n, steps), -1, dtype=numpy.int64), 'status': numpy.zeros(n, dtype=numpy.int32),
           'exit_step': numpy.full(n, steps, dtype=numpy.int32)}
    out['theta'][:, 0] = theta0
    th = theta0.copy()
    running = numpy.ones(n, dtype=bool)
    bits, traj_steps = 0, 0
    for k in range(steps):
        bad = running & ~numpy.all(numpy.isfinite(th), axis=1)
        out['status'][bad], out['exit_step'][bad] = 3, k
        running &= ~bad
        idx = numpy.flatnonzero(running)
        if idx.size == 0:
            break
        traj_steps += idx.size
        row_bits, _, obj_bits = lref.exact_bits(ef, xlaw, th[idx], tol, Q, cvec, H)
        bits = max(bits, row_bits, obj_bits if overlapping else 0)
        assert bits <= 53, (k, row_bits, obj_bits)
        region = lref.locate(row_off, ef, xlaw, th[idx], tol, overlapping, inclusive, Q, cvec, H)[0]
        none = region < 0
        out['status'][idx[none]], out['exit_step'][idx[none]] = 2, k
        running[idx[none]] = False
        idx, region = idx[~none], region[~none]
        if idx.size == 0:
            break
        tI, et = _ints(th[idx])
        tabs = _absI(tI)
        # u = b + L theta in units of 2^(eL + et)
        eu = eL + et
        uI, umag = numpy.empty((idx.size, nu), dtype=object), numpy.empty((idx.size, nu), dtype=object)
        for r in numpy.unique(region):
            sel = region == r
            b, L = LI[r][:, 0] * (1 << -et), LI[r][:, 1:]
            uI[sel] = numpy.dot(tI[sel], L.T) + b
            umag[sel] = numpy.dot(tabs[sel], _absI(L).T) + _absI(b)
        u, ub = _floats(uI, eu, umag)
        # theta+ = c + A theta + B u + w in units of 2^en
        en = min(ec, eA + et, eB + eu, ew)
        sc, sa, sb, sw = (1 << (ec - en)), (1 << (eA + et - en)), (1 << (eB + eu - en)), (1 << (ew - en))
        nI = numpy.dot(tI, AI.T) * sa + numpy.dot(uI, BI.T) * sb + cI * sc + wI[idx, k] * sw
        nmag = numpy.dot(tabs, _absI(AI).T) * sa + numpy.dot(_absI(uI), _absI(BI).T) * sb + _absI(cI) * sc + _absI(wI[idx, k]) * sw
        nxt, nb = _floats(nI, en, nmag)
        dI = nI - tI * (1 << (et - en))
        diff, db = _floats(dI, en, _absI(nI) + tabs * (1 << (et - en)))
        bits = max(bits, ub, nb, db)
        out['region'][idx, k], out['u'][idx, k], out['theta'][idx, k + 1] = region, u, nxt
        th[idx] = nxt
        if stop_tol is not None:
            steady = numpy.all(numpy.abs(diff) <= stop_tol, axis=1)
            out['status'][idx[steady]], out['exit_step'][idx[steady]] = 1, k + 1
            running[idx[steady]] = False
    out['bits'], out['traj_steps'] = bits, traj_steps
    return out


# ---- lattice plants ----------------------------------------------------------------------------------------------------------------
def _sparse_rows(rng, rows, cols, values, per_row=2):
    """[rows, cols]: per row `per_row` entries (fewer when cols is smaller) drawn from `values`, zeros elsewhere"""
    M = numpy.zeros((rows, cols))
    for i in range(rows):
        at = rng.choice(cols, size=min(per_row, cols), replace=False)
        M[i, at] = rng.choice(values, size=len(at))
    return M


QUARTERS = numpy.array([-0.5, -0.25, 0.25, 0.5])


def lattice_laws(rng, R, n_x, n_t):
    """laws [R, n_x, n_t + 1] = [b | A]: b on the 1/4 lattice in [-1, 1], two entries of +-1/4 / +-1/2 per row of A"""
    laws = numpy.zeros((R, n_x, n_t + 1))
    laws[:, :, 0] = lref.lattice(rng, (R, n_x), -1.0, 1.0, 0.25)
    laws[:, :, 1:] = _sparse_rows(rng, R * n_x, n_t, QUARTERS).reshape(R, n_x, n_t)
    return laws


def lattice_plant(rng, n_t, n_u, n_x, with_c=True, diag=0.5):
    """dict of A = diag I (I / 2) plus one off-diagonal +-1/4 per row, B with two entries of +-1/4 / +-1/2 per row, c on the 1/4 lattice in
    [-1/2, 1/2] (or None) and `inputs`: n_u rows of the law in no order, one of them twice when n_u >= 2"""
    A = diag * numpy.eye(n_t)
    for i in range(n_t):
        if n_t > 1:
            A[i, (i + 1 + int(rng.integers(n_t - 1))) % n_t] = rng.choice([-0.25, 0.25])
    inputs = [int(i) for i in rng.permutation(n_x)[:n_u]]
    if n_u >= 2:
        inputs[-1] = inputs[0]
    return {'A': A, 'B': _sparse_rows(rng, n_t, n_u, QUARTERS), 'c': lref.lattice(rng, n_t, -0.5, 0.5, 0.25) if with_c else None,
            'inputs': inputs}


def lattice_starts(rng, n, n_t, tol, reach=3.5, edge=4.0):
    """theta_0 [n, n_t] on the 1/16 lattice in [-reach, reach]; one start in twenty sits at edge + tol on one axis (on the outer box of
    a Grid: outside by the strict rule, inside by the inclusive one)"""
    th = lref.lattice(rng, (n, n_t), -reach, reach, 0.0625)
    for p in numpy.flatnonzero(rng.random(n) < 0.05):
        th[p, int(rng.integers(n_t))] = edge + tol
    return th


def lattice_disturbance(rng, n, steps, n_t):
    """w [n, steps, n_t] on the 1/8 lattice in [-1/4, 1/4]"""
    return lref.lattice(rng, (n, steps, n_t), -0.25, 0.25, 0.125)


def count_steps(status, exit_step, steps):
    """steps taken by trajectories with these ends, as mpc_sim_stats.traj_steps counts them: the step that finds no region counts, the
    visit that finds a non-finite state does not"""
    status, exit_step = numpy.asarray(status), numpy.asarray(exit_step)
    return int(numpy.sum(numpy.where(status == 0, steps, exit_step + (status == 2))))


def step_in_order(theta, u, A, B, c=None, w=None):
    """theta+ of many states [m, n_t] with inputs [m, n_u] in the documented order of the device: c (or 0.0), the A terms, the B terms,
    then w, every product and every sum rounded on its own (numpy fuses nothing).  For data that do round."""
    theta, u = numpy.asarray(theta, dtype=float), numpy.asarray(u, dtype=float)
    A, B = numpy.asarray(A, dtype=float), numpy.asarray(B, dtype=float).reshape(len(A), -1)
    out = numpy.empty_like(theta)
    for i in range(A.shape[0]):
        v = numpy.full(len(theta), 0.0 if c is None else float(c[i]))
        for j in range(A.shape[1]):
            v = v + A[i, j] * theta[:, j]
        for l in range(B.shape[1]):
            v = v + B[i, l] * u[:, l]
        if w is not None:
            v = v + w[:, i]
        out[:, i] = v
    return out
