"""Host reference for closed-loop simulation (Solution.simulate): a plain loop over Solution.get_region and
CriticalRegion.evaluate, the way the reference's MPC tutorial steps an explicit controller.  No device, no code of ppopt_amd.closed_loop.
A plain helper module (not a conftest), imported by tests/test_closed_loop_cpu.py and tests/test_gpu_closed_loop.py."""
import numpy


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
