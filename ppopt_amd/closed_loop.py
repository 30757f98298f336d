"""Explicit controllers in closed loop on the device: ``simulate(solution, theta0, steps, A, B, inputs, ...)`` runs many
trajectories of theta+ = A theta + B u + c + w under the law u = x*(theta)[inputs] in one launch (k_simulate, csrc/closed_loop.hpp).

One step of trajectory p at theta_k: j_k = ``solution.get_region_batch(theta_k)`` (the same tolerance and rule); j_k = -1 ends the
trajectory (status 2); u_k = ``solution.evaluate_batch(theta_k)[0][:, inputs]`` bit for bit; theta_{k+1} component i is formed in
the order ``v = c_i; v = v + A_i0 theta_0; ...; v = v + B_i0 u_0; ...; v = v + w_i`` with one rounding per product and per sum (no
fma), so that ``replay_step`` reproduces it bit for bit.  ``disturbance_box`` replays the device's box draw.
"""
from dataclasses import dataclass, field
from typing import Optional

import numpy

__all__ = ['ClosedLoopResult', 'simulate', 'disturbance_box', 'replay_step', 'RAN', 'STEADY', 'LEFT', 'NON_FINITE']

RAN, STEADY, LEFT, NON_FINITE = 0, 1, 2, 3      # statuses: all steps ran; |theta+ - theta|_inf <= stop_tol; no region; non-finite state
LOCATE_MODES = ('auto', 'tree', 'walk', 'scan')
_MASK = numpy.uint64(0xffffffff)


@dataclass
class ClosedLoopResult:
    """theta [n, steps+1, n_theta] (float64; with record='final' [n, n_theta], the state at exit_step); u [n, steps, n_u]; region
    [n, steps] int64; status [n] int32 (RAN, STEADY, LEFT, NON_FINITE); exit_step [n] int32, the index of the last state.  After a
    trajectory's end theta and u are NaN and region is -1; u and region are None with record='final'."""
    theta: numpy.ndarray
    u: Optional[numpy.ndarray]
    region: Optional[numpy.ndarray]
    status: numpy.ndarray
    exit_step: numpy.ndarray
    stats: dict = field(default_factory=dict)


# ---- the box disturbance, replayed on the host ------------------------------------------------------------------------------------
def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Random123 constants) of counter arrays (broadcast) under the key (k0, k1): four uint64 arrays of 32-bit words."""
    c = [numpy.asarray(v, dtype=numpy.uint64) & _MASK for v in numpy.broadcast_arrays(c0, c1, c2, c3)]
    k = [numpy.uint64(k0), numpy.uint64(k1)]
    for r in range(10):
        if r:
            k = [(k[0] + numpy.uint64(0x9E3779B9)) & _MASK, (k[1] + numpy.uint64(0xBB67AE85)) & _MASK]
        lo0 = numpy.uint64(0xD2511F53) * c[0]
        lo1 = numpy.uint64(0xCD9E8D57) * c[2]
        c = [((lo1 >> numpy.uint64(32)) ^ c[1] ^ k[0]) & _MASK, lo1 & _MASK, ((lo0 >> numpy.uint64(32)) ^ c[3] ^ k[1]) & _MASK, lo0 & _MASK]
    return c


def _u53(a, b):
    return ((a >> numpy.uint64(5)).astype(numpy.float64) * 67108864.0 + (b >> numpy.uint64(6)).astype(numpy.float64)) * 2.0 ** -53


def sim_key(seed: int):
    """The Philox key of a run: (seed mod 2^32, (seed >> 32) xor MPC_SIM_KEY_SALT)."""
    from ._lib import MPC_SIM_KEY_SALT
    seed = int(seed)
    return seed & 0xffffffff, ((seed >> 32) ^ MPC_SIM_KEY_SALT) & 0xffffffff


def disturbance_box(seed: int, n: int, steps: int, lo, hi) -> numpy.ndarray:
    """The box disturbance the device draws for ``simulate(..., disturbance=(lo, hi), seed=seed)``: w [n, steps, n_theta] with
    w[p, k, i] = lo_i + (hi_i - lo_i) U, U = u53 of Philox4x32-10 at the counter (p mod 2^32, p >> 32, k, i // 2), words (0, 1) for
    even i and (2, 3) for odd i."""
    lo, hi = numpy.asarray(lo, dtype=numpy.float64).reshape(-1), numpy.asarray(hi, dtype=numpy.float64).reshape(-1)
    nt = len(lo)
    k0, k1 = sim_key(seed)
    p = numpy.arange(int(n), dtype=numpy.uint64)[:, None]
    k = numpy.arange(int(steps), dtype=numpy.uint64)[None, :]
    w = numpy.empty((int(n), int(steps), nt))
    for j in range((nt + 1) // 2):
        r = _philox4x32_10(p & _MASK, p >> numpy.uint64(32), k, j, k0, k1)
        for i, (a, b) in ((2 * j, (r[0], r[1])), (2 * j + 1, (r[2], r[3]))):
            if i < nt:
                w[:, :, i] = lo[i] + (hi[i] - lo[i]) * _u53(a, b)
    return w


def replay_step(theta, u, A, B, c=None, w=None) -> numpy.ndarray:
    """theta_{k+1} of many states at once, in the device's order: c (or 0.0), then A_i0 theta_0 ..., then B_i0 u_0 ..., then w_i (when
    given), each product and each sum rounded on its own."""
    theta, u = numpy.atleast_2d(numpy.asarray(theta, dtype=numpy.float64)), numpy.atleast_2d(numpy.asarray(u, dtype=numpy.float64))
    A, B = numpy.asarray(A, dtype=numpy.float64), numpy.asarray(B, dtype=numpy.float64).reshape(len(A), -1)
    nt = A.shape[0]
    out = numpy.empty_like(theta)
    for i in range(nt):
        v = numpy.full(len(theta), 0.0 if c is None else float(numpy.asarray(c, dtype=numpy.float64).reshape(-1)[i]))
        for j in range(nt):
            v = v + A[i, j] * theta[:, j]
        for l in range(B.shape[1]):
            v = v + B[i, l] * u[:, l]
        if w is not None:
            v = v + numpy.atleast_2d(w)[:, i]
        out[:, i] = v
    return out


# ---- validation (before any device call) -----------------------------------------------------------------------------------------
def _law_rows(solution, n_t: int) -> int:
    """rows of the law the locator holds: x of a continuous region, the full variable vector of a mixed-integer one, the merged rows"""
    r = solution.critical_regions[0]
    if getattr(r, 'y_fixation', None) is not None:
        return len(r.x_indices) + len(r.y_indices)
    return numpy.asarray(r.A).reshape(-1, n_t).shape[0]


def _finite(name, a):
    if not numpy.all(numpy.isfinite(a)):
        raise ValueError(f'simulate: {name} must be finite')
    return a


def _check(solution, theta0, steps, A, B, inputs, c, disturbance, seed, stop_tol, locate, record, budget):
    from ._lib import SIM_DEFAULT_BUDGET, SIM_MAX_DIM, SIM_MAX_INPUTS
    if not solution.critical_regions:
        raise ValueError('simulate: the solution has no region')
    n_t = solution.program.num_t() if solution.program is not None else numpy.asarray(solution.critical_regions[0].E).shape[1]
    if n_t > SIM_MAX_DIM:
        raise ValueError(f'simulate: n_theta = {n_t} > {SIM_MAX_DIM}')
    if locate not in LOCATE_MODES:
        raise ValueError(f'simulate: locate must be one of {LOCATE_MODES}, not {locate!r}')
    if record not in ('full', 'final'):
        raise ValueError(f"simulate: record must be 'full' or 'final', not {record!r}")
    if isinstance(steps, bool) or int(steps) != steps or not 1 <= int(steps) <= 1 << 30:
        raise ValueError(f'simulate: steps must be an integer in 1..2^30, not {steps!r}')
    steps = int(steps)
    th0 = numpy.asarray(theta0, dtype=numpy.float64)
    if th0.ndim == 1:
        th0 = th0.reshape(1, -1)
    if th0.ndim != 2 or th0.shape[1] != n_t:
        raise ValueError(f'simulate: theta0 must be [n, {n_t}], not {list(numpy.shape(theta0))}')
    _finite('theta0', th0)
    A = numpy.asarray(A, dtype=numpy.float64)
    if A.shape != (n_t, n_t):
        raise ValueError(f'simulate: A must be [{n_t}, {n_t}], not {list(A.shape)}')
    B = numpy.asarray(B, dtype=numpy.float64)
    if B.ndim == 1 and len(B) == n_t:
        B = B.reshape(n_t, 1)
    if B.ndim != 2 or B.shape[0] != n_t:
        raise ValueError(f'simulate: B must be [{n_t}, n_u], not {list(B.shape)}')
    n_u = B.shape[1]
    if not 1 <= n_u <= SIM_MAX_INPUTS:
        raise ValueError(f'simulate: n_u = {n_u} must lie in 1..{SIM_MAX_INPUTS}')
    inp = numpy.asarray(inputs).reshape(-1)
    if len(inp) != n_u or not numpy.issubdtype(inp.dtype, numpy.integer):
        raise ValueError(f'simulate: inputs must be {n_u} integer indices (one per column of B)')
    n_x = _law_rows(solution, n_t)
    if inp.min() < 0 or inp.max() >= n_x:
        raise ValueError(f'simulate: inputs {inp.tolist()} out of range: the law has {n_x} rows')
    _finite('A', A)
    _finite('B', B)
    if c is not None:
        c = numpy.asarray(c, dtype=numpy.float64).reshape(-1)
        if len(c) != n_t:
            raise ValueError(f'simulate: c must have {n_t} entries')
        _finite('c', c)
    n = len(th0)
    w = box = None
    if disturbance is not None:
        if isinstance(disturbance, (tuple, list)) and len(disturbance) == 2:
            lo, hi = (numpy.asarray(v, dtype=numpy.float64).reshape(-1) for v in disturbance)
            if len(lo) != n_t or len(hi) != n_t:
                raise ValueError(f'simulate: the box (lo, hi) needs two vectors of {n_t} entries')
            _finite('the box', numpy.concatenate([lo, hi]))
            if numpy.any(lo > hi):
                raise ValueError('simulate: the box needs lo <= hi')
            box = (lo, hi)
        else:
            w = numpy.asarray(disturbance, dtype=numpy.float64)
            if w.shape != (n, steps, n_t):
                raise ValueError(f'simulate: a disturbance array must be [{n}, {steps}, {n_t}], not {list(w.shape)}')
            _finite('the disturbance', w)
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 1 << 64:
        raise ValueError('simulate: seed must be an integer in 0..2^64-1')
    if stop_tol is not None and not (numpy.isfinite(stop_tol) and stop_tol >= 0):
        raise ValueError('simulate: stop_tol must be None or finite and >= 0')
    cap = int(budget) if budget and budget > 0 else SIM_DEFAULT_BUDGET
    rec = n * n_t * 8 if record == 'final' else n * ((steps + 1) * n_t * 8 + steps * (n_u * 8 + 4))
    need = rec + n * n_t * 8 + (n * steps * n_t * 8 if w is not None else 0)
    if need > cap:
        raise ValueError(f"simulate: the run needs {need} device bytes, more than the budget of {cap}: use record='final' or fewer trajectories")
    return th0, steps, A, B, inp.astype(numpy.int32), c, w, box, n_t


def simulate(solution, theta0, steps: int, A, B, inputs, c=None, disturbance=None, seed: int = 0, stop_tol: Optional[float] = None,
             locate: str = 'auto', record: str = 'full', inclusive: bool = False, device: int = 0, budget: int = 0) -> ClosedLoopResult:
    """Closed-loop trajectories of the explicit controller ``solution`` on the plant theta+ = A theta + B u + c + w, u = x*(theta)[inputs],
    from every row of theta0, for ``steps`` steps, in one device launch (module docstring).

    disturbance: None, an array [n, steps, n_theta], or a box ``(lo, hi)`` drawn on the device (``disturbance_box(seed, ...)``).
    stop_tol: a trajectory with |theta_{k+1} - theta_k|_inf <= stop_tol ends (status STEADY).  locate: 'tree' (``solution.search_tree()``),
    'walk' (the adjacency walk from the previous region; complete, non-overlapping solutions with adjacency, not inclusive), 'scan', or
    'auto' (an attached tree of tolerance >= point_location_tolerance, else the walk where it is allowed, else the scan).  record:
    'full' or 'final' (the state at exit_step only).  budget: device bytes (<= 0: 4 GiB).  ValueError before any device call for bad
    arguments; MpcError from the library."""
    th0, steps, A, B, inp, c, w, box, n_t = _check(solution, theta0, steps, A, B, inputs, c, disturbance, seed, stop_tol, locate, record,
                                                   budget)
    overlapping = bool(solution.is_overlapping)
    walk_allowed = bool(solution.use_walk and solution.is_complete and not overlapping and not inclusive)
    if locate == 'walk' and not walk_allowed:
        raise ValueError('simulate: the walk needs a complete, non-overlapping solution and inclusive=False')
    loc = solution.locator(device)
    tol = solution.point_location_tolerance
    mode = locate
    if locate == 'tree':
        tree = solution.search_tree() if device == 0 else solution.search_tree(device=device)
        loc = tree._locator(device)
    elif locate == 'auto':
        owner = getattr(loc, 'tree_owner', None)
        if owner is not None and owner.tol >= tol:
            mode = 'tree'
        elif walk_allowed and loc.has_adjacency:
            mode = 'walk'
        else:
            mode = 'scan'
    if mode == 'walk' and not loc.has_adjacency:
        raise ValueError(f'simulate: the walk needs facet adjacency, which the locator holds only for device-solved solutions of at least '
                         f'{solution.WALK_MIN_REGIONS} regions')
    final = record == 'final'
    w_s = None if w is None else numpy.ascontiguousarray(w.transpose(1, 0, 2))
    theta, u, region, status, exit_step, st = loc.simulate(th0, steps, A, B, inp, c=c, w=w_s, box=box, seed=int(seed), tol=tol,
                                                           stop_tol=stop_tol, overlapping=overlapping, inclusive=inclusive,
                                                           walk=mode == 'walk', tree=mode == 'tree', final_only=final, budget=budget)
    n = len(th0)
    stats = {'mode': mode, 'ms': float(st['ms']), 'trajectory_steps': int(st['traj_steps']), 'crossings': int(st['crossings']),
             'fallbacks': int(st['fallbacks']), 'crossings_per_step': st['crossings'] / st['traj_steps'] if st['traj_steps'] else 0.0,
             'status_counts': numpy.bincount(status, minlength=4).tolist(), 'n': n, 'steps': steps}
    if final:
        return ClosedLoopResult(theta=theta, u=None, region=None, status=status, exit_step=exit_step, stats=stats)
    return ClosedLoopResult(theta=numpy.ascontiguousarray(theta.transpose(1, 0, 2)), u=numpy.ascontiguousarray(u.transpose(1, 0, 2)),
                            region=region.T.astype(numpy.int64), status=status, exit_step=exit_step, stats=stats)
