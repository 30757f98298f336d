"""Recursive feasibility of an explicit controller in closed loop, certified region by region.

Let Theta_f be the parameters where the program is feasible: a projection of a polyhedron, so convex for a continuous mpLP or mpQP.  On
region i the loop is affine, theta+ = Phi_i theta + phi_i with Phi_i = A + B A_i[inputs] and phi_i = B b_i[inputs] + c, so the image of
the region is the convex hull of the images of its vertices, and it lies in Theta_f exactly when every image vertex is feasible (with a
box disturbance: every image vertex plus every box corner).  Each image point theta+ is checked by one device LP, the margin LP

    min s  s.t.  A x <= b + F theta+ + s (1 + |b + F theta+|)  (inequality rows),  the equality rows exact,
                 A_t theta+ <= b_t + s (1 + |b_t|),  s >= -1,

whose optimum s* <= tol says theta+ is feasible (within tol, relative to the rows' right-hand sides); an infeasible LP is +inf.
"""
import time
from dataclasses import dataclass, field
from itertools import product

import numpy

from . import _lib

__all__ = ['FeasibilityCertificate', 'certify_recursive_feasibility', 'image_points', 'margin_lp_rows', 'INSIDE', 'LEAVES', 'UNDECIDED']

INSIDE, LEAVES, UNDECIDED = 0, 1, 2
LP_BATCH_BYTES = 256 << 20      # host bytes of one device batch of margin LPs (Solver.MILP_BATCH_BYTES)
MAX_BOX_DIM = 10                # a box disturbance has 2^n_theta corners per vertex


@dataclass
class FeasibilityCertificate:
    """margin [n_regions]: the largest s* over the region's image points (NaN where undecided); status [n_regions]: INSIDE (margin <= tol),
    LEAVES, UNDECIDED (the vertex pass gave UNBOUNDED, NOT_POINTED, EMPTY or OVERFLOW, or a margin LP hit its iteration limit);
    witness_theta / witness_image [n_regions, n_theta]: for leaving regions the vertex and the image point of the largest margin (NaN
    elsewhere); certified: every region INSIDE; stats: vertex ms, LP ms, LPs."""
    margin: numpy.ndarray
    status: numpy.ndarray
    witness_theta: numpy.ndarray
    witness_image: numpy.ndarray
    certified: bool
    stats: dict = field(default_factory=dict)


def _finite(name, a, who='certify_recursive_feasibility'):
    if not numpy.all(numpy.isfinite(a)):
        raise ValueError(f'{who}: {name} must be finite')
    return a


def _check(solution, A, B, inputs, c, disturbance, tol, who='certify_recursive_feasibility'):
    """The argument checks certify_recursive_feasibility and transition.transition_graph (``who``) share."""
    from .closed_loop import _law_rows
    if not solution.critical_regions:
        raise ValueError(f'{who}: the solution has no region')
    if getattr(solution.critical_regions[0], 'y_fixation', None) is not None or hasattr(solution.program, 'binary_indices'):
        raise ValueError(f'{who}: a mixed-integer solution is refused: its feasible parameter set need not be convex')
    n_t = solution.program.num_t() if solution.program is not None else numpy.asarray(solution.critical_regions[0].E).shape[1]
    A = numpy.asarray(A, dtype=numpy.float64)
    if A.shape != (n_t, n_t):
        raise ValueError(f'{who}: A must be [{n_t}, {n_t}], not {list(A.shape)}')
    B = numpy.asarray(B, dtype=numpy.float64)
    if B.ndim == 1 and len(B) == n_t:
        B = B.reshape(n_t, 1)
    if B.ndim != 2 or B.shape[0] != n_t or B.shape[1] < 1:
        raise ValueError(f'{who}: B must be [{n_t}, n_u], not {list(B.shape)}')
    n_u = B.shape[1]
    inp = numpy.asarray(inputs).reshape(-1)
    if len(inp) != n_u or not numpy.issubdtype(inp.dtype, numpy.integer):
        raise ValueError(f'{who}: inputs must be {n_u} integer indices (one per column of B)')
    n_x = _law_rows(solution, n_t)
    if inp.min() < 0 or inp.max() >= n_x:
        raise ValueError(f'{who}: inputs {inp.tolist()} out of range: the law has {n_x} rows')
    _finite('A', A, who)
    _finite('B', B, who)
    if c is not None:
        c = numpy.asarray(c, dtype=numpy.float64).reshape(-1)
        if len(c) != n_t:
            raise ValueError(f'{who}: c must have {n_t} entries')
        _finite('c', c, who)
    box = None
    if disturbance is not None:
        if not (isinstance(disturbance, (tuple, list)) and len(disturbance) == 2):
            raise ValueError(f'{who}: the disturbance must be None or a box (lo, hi)')
        lo, hi = (numpy.asarray(v, dtype=numpy.float64).reshape(-1) for v in disturbance)
        if len(lo) != n_t or len(hi) != n_t:
            raise ValueError(f'{who}: the box (lo, hi) needs two vectors of {n_t} entries')
        _finite('the box', numpy.concatenate([lo, hi]), who)
        if numpy.any(lo > hi):
            raise ValueError(f'{who}: the box needs lo <= hi')
        if n_t > MAX_BOX_DIM:
            raise ValueError(f'{who}: a box disturbance needs n_theta <= {MAX_BOX_DIM} (2^n_theta corners per vertex), not {n_t}')
        box = (lo, hi)
    if not (numpy.isfinite(tol) and tol >= 0):
        raise ValueError(f'{who}: tol must be finite and >= 0')
    return A, B, inp.astype(numpy.int64), c, box, n_t


def closed_loop_maps(xlaw, A, B, inputs, c=None):
    """(Phi [n_regions, n_t, n_t], phi [n_regions, n_t]) of the laws xlaw [n_regions, n_x, n_t + 1] = [b | A]: Phi_i = A + B A_i[inputs],
    phi_i = B b_i[inputs] + c."""
    law = numpy.asarray(xlaw, dtype=numpy.float64)[:, inputs, :]          # [n, n_u, n_t + 1]
    Phi = A[None] + numpy.einsum('tu,nuk->ntk', B, law[:, :, 1:])
    phi = numpy.einsum('tu,nu->nt', B, law[:, :, 0]) + (0.0 if c is None else numpy.asarray(c, dtype=numpy.float64)[None])
    return Phi, phi


def box_corners(lo, hi) -> numpy.ndarray:
    """[2^n, n]: every corner of the box, lo / hi chosen by the bits of the corner index (bit j: component j takes hi)"""
    lo, hi = numpy.asarray(lo, dtype=numpy.float64), numpy.asarray(hi, dtype=numpy.float64)
    bits = numpy.array(list(product((0, 1), repeat=len(lo))))[:, ::-1].astype(bool)
    return numpy.where(bits, hi[None], lo[None])


def image_points(vertices, region_of_vertex, Phi, phi, box=None):
    """(image points [V * K, n_t], the vertex of each [V * K]): Phi_i v + phi_i of every vertex v of region i, plus every box corner
    (K = 2^n_t corners, or K = 1 without a box), vectorised over all vertices at once."""
    V = numpy.asarray(vertices, dtype=numpy.float64)
    reg = numpy.asarray(region_of_vertex, dtype=numpy.int64)
    img = numpy.einsum('vtk,vk->vt', Phi[reg], V) + phi[reg]
    if box is None:
        return img, numpy.arange(len(V))
    corners = box_corners(*box)
    pts = (img[:, None, :] + corners[None]).reshape(-1, V.shape[1])
    return pts, numpy.repeat(numpy.arange(len(V)), len(corners))


def margin_lp_rows(program, theta_plus):
    """The margin LPs of the image points theta_plus [k, n_t] over the program's rows: (A3 [k, m, n_x + 1], b2 [k, m], eq flags [m],
    c [n_x + 1]) with the variables (x, s).  Rows: the program's rows A x - s (1 + |b + F theta+|) <= b + F theta+ (equality rows: s
    coefficient 0, flagged), then -s (1 + |b_t|) <= b_t - A_t theta+, then -s <= 1."""
    P = program
    Ax, b, F = numpy.asarray(P.A, dtype=float), numpy.asarray(P.b, dtype=float).reshape(-1), numpy.asarray(P.F, dtype=float)
    At, bt = numpy.asarray(P.A_t, dtype=float), numpy.asarray(P.b_t, dtype=float).reshape(-1)
    th = numpy.atleast_2d(numpy.asarray(theta_plus, dtype=float))
    k, (mc, nx), mt = len(th), Ax.shape, len(bt)
    eq = numpy.zeros(mc + mt + 1, dtype=numpy.uint8)
    eq[list(P.equality_indices)] = 1
    rhs = b[None] + th @ F.T                                    # [k, mc]
    A3 = numpy.zeros((k, mc + mt + 1, nx + 1))
    A3[:, :mc, :nx] = Ax[None]
    A3[:, :mc, nx] = numpy.where(eq[:mc] == 1, 0.0, -(1.0 + numpy.abs(rhs)))
    A3[:, mc:mc + mt, nx] = -(1.0 + numpy.abs(bt))[None]
    A3[:, mc + mt, nx] = -1.0
    b2 = numpy.empty((k, mc + mt + 1))
    b2[:, :mc] = rhs
    b2[:, mc:mc + mt] = bt[None] - th @ At.T
    b2[:, mc + mt] = 1.0
    cvec = numpy.zeros(nx + 1)
    cvec[nx] = 1.0
    return A3, b2, eq, cvec


def margins(program, theta_plus, device: int = 0):
    """(s* [k]: +inf where the margin LP is infeasible, NaN where it did not finish, LPs solved, host seconds of the LP batches) of
    the image points, in device batches of at most LP_BATCH_BYTES (every LP carries its own copy of the matrix)."""
    th = numpy.atleast_2d(numpy.asarray(theta_plus, dtype=float))
    out = numpy.empty(len(th))
    m = len(numpy.asarray(program.b).reshape(-1)) + len(numpy.asarray(program.b_t).reshape(-1)) + 1
    n = program.A.shape[1] + 1
    per_lp = 8 * (m * n + m) + m
    step = max(1, int(LP_BATCH_BYTES // per_lp))
    seconds = 0.0
    for first in range(0, len(th), step):
        A3, b2, eq, cvec = margin_lp_rows(program, th[first:first + step])
        t0 = time.perf_counter()
        status, _, obj, _ = _lib.lp_solve_batch(A3, b2, cvec, numpy.broadcast_to(eq, b2.shape), device=device, want_x=False)
        seconds += time.perf_counter() - t0
        out[first:first + step] = numpy.where(status == _lib.LP_OPTIMAL, obj,
                                              numpy.where(status == _lib.LP_INFEASIBLE, numpy.inf, numpy.nan))
    return out, len(th), seconds


def certify_recursive_feasibility(solution, A, B, inputs, c=None, disturbance=None, tol: float = 1e-7, device: int = 0) -> FeasibilityCertificate:
    """Whether the explicit controller ``solution`` keeps the plant theta+ = A theta + B u + c (+ w, w in the box ``disturbance``),
    u = x*(theta)[inputs], where the program is feasible: the module docstring's certificate, region by region.

    A region's verdict is about that region's own law: INSIDE means every point of the region (closed) maps, under its law, to a point
    where the program is feasible.  If every region passes, the controller is recursively feasible on the union of its regions,
    whichever region the locator picks.  In a non-overlapping solution, a LEAVING region means that interior points near the witness
    also leave.  ValueError before any launch for mixed-integer solutions (their Theta_f need not be convex), A that is not
    n_theta x n_theta, B and inputs of the wrong shape, non-finite arguments, a box with lo > hi and a box in more than 10 dimensions."""
    A, B, inp, c, box, n_t = _check(solution, A, B, inputs, c, disturbance, tol)
    rv = solution.vertices(device=device)
    _, _, xlaw = solution._stacked()
    Phi, phi = closed_loop_maps(xlaw, A, B, inp, c)
    n_reg = len(rv.status)
    region_of_vertex = numpy.repeat(numpy.arange(n_reg), numpy.diff(rv.offsets))
    pts, vert_of_pt = image_points(rv.vertices, region_of_vertex, Phi, phi, box)
    s, n_lps, lp_seconds = margins(solution.program, pts, device=device) if len(pts) else (numpy.zeros(0), 0, 0.0)
    margin = numpy.full(n_reg, numpy.nan)
    status = numpy.full(n_reg, UNDECIDED, dtype=numpy.int32)
    wt, wi = numpy.full((n_reg, n_t), numpy.nan), numpy.full((n_reg, n_t), numpy.nan)
    reg_of_pt = region_of_vertex[vert_of_pt]
    ok = rv.status == _lib.VX_OK
    if len(pts):
        # the largest margin of every region (NaN -- an LP that did not finish -- leaves the region undecided)
        key = numpy.where(numpy.isnan(s), numpy.inf, s)
        order = numpy.lexsort((-key, reg_of_pt))
        first = numpy.unique(reg_of_pt[order], return_index=True)
        regs, at = first[0], order[first[1]]
        has_nan = numpy.zeros(n_reg, dtype=bool)
        has_nan[reg_of_pt[numpy.isnan(s)]] = True
        margin[regs] = s[at]
        decided = ok[regs] & ~has_nan[regs]
        r_in = regs[decided & (s[at] <= tol)]
        r_out = regs[decided & ~(s[at] <= tol)]
        status[r_in] = INSIDE
        status[r_out] = LEAVES
        leave_at = at[decided & ~(s[at] <= tol)]
        wt[r_out] = rv.vertices[vert_of_pt[leave_at]]
        wi[r_out] = pts[leave_at]
        margin[~ok] = numpy.nan
    stats = {'vertex_ms': float(rv.stats['ms']), 'lp_ms': 1e3 * lp_seconds, 'lps': int(n_lps),
             'status_counts': numpy.bincount(status, minlength=3).tolist()}
    return FeasibilityCertificate(margin=margin, status=status, witness_theta=wt, witness_image=wi, certified=bool(numpy.all(status == INSIDE)),
                                  stats=stats)
