"""Projecting polytopes on the device: elimination of coordinates, affine images, Minkowski sums, one-step controllable sets.

A polytope P of R^n is given as unit rows [o | n] (|n| = 1, {x : n.x <= o}), m rows in order; ``tol`` has the meaning of §3.19 to §3.23: a
set whose Chebyshev radius is not above tol does not count.  The trailing n_elim coordinates are eliminated one at a time, the last one
first (Fourier-Motzkin), and after every step the rows that the step made in excess are removed by the sequential rule of §3.22.

  thin test     the radius run over the rows from the start point (the origin without one), stopped once t > tol.  Optimal with t <= tol:
                THIN, no rows.  Otherwise the point where the run ended is the interior point.
  one step      from dimension d to d - 1, coordinate j = d - 1, over the live rows in order.  c is a row's coefficient of j;
                Z: |c| <= 1e-12, P: c > 1e-12, N: c < -1e-12.  The new rows: the rows of Z in order without column j (scaled to a unit
                normal again unless c == 0: only then has the norm changed), then for p over P in order and q over N in order inside it
                (-c_q) row_p + c_p row_q without column j, scaled to a unit normal over the d - 1 coordinates left.
  zero rows     a combination whose normal has a norm <= 1e-9 before scaling says 0 <= rhs: with rhs >= -tol it is dropped, otherwise
                the polytope is empty: THIN.
  empty P or N  the step keeps the rows of Z alone.  No row left (here or after the zero rows): WHOLE, the whole space, no rows.
  row limit     |Z| + |P||N| > 512: TOO_LARGE, no rows; never a partial result.  ``peak`` is the largest such count of a polytope.
  reduce        the interior point loses coordinate j (it is interior to the projection), the thin test from it (t <= tol: THIN;
                otherwise the point moves to where the run ended, which is where it started whenever it was interior), then the
                sequential rule of §3.22 over the new rows.  The kept rows, in order, are the live rows of the next step.  Unbounded or
                capped runs count as kept and add to ``wide``.
  the end       the live rows are the result; more than out_cap of them: TOO_LARGE.  n_elim = 0 is one pass of reduce_rows_of.

What follows: in exact arithmetic the rows before each reduce describe the projection exactly, and the reduce never loses a point, so the
result contains proj(P) and every removed row cut off a set of radius <= tol at its removal; the result is deterministic and depends on
the row order and on the elimination order; a full-dimensional bounded P gives a result without a redundant row.  Every step runs on the
device (csrc/project.hpp, k_project_rows, one wavefront per polytope): n <= 16, at most 512 rows at every step; the row count of the
elimination grows exponentially in the worst case.
"""
import time
from dataclasses import dataclass, field
from typing import Optional, Sequence, Union

import numpy

from .polytope import Polytope
from .reduce import check_rows, polytope_unit_rows

__all__ = ['ProjectedRows', 'project_rows_of', 'project_polytopes', 'affine_image', 'minkowski_sum', 'controllable_pre', 'MAX_ROWS', 'MAX_DIM',
           'OK', 'THIN', 'WHOLE', 'TOO_LARGE', 'STATUS']

MAX_ROWS = 512    # PJ_MAX_ROWS of csrc/project.hpp
MAX_DIM = 16
OK, THIN, WHOLE, TOO_LARGE = range(4)   # status of a polytope (MPC_PROJECT_*)
STATUS = ('OK', 'THIN', 'WHOLE', 'TOO_LARGE')


@dataclass
class ProjectedRows:
    """The projections in CSR form: polytope q has rows[row_off[q]:row_off[q + 1]], unit rows [o | n] over the kept coordinates in the
    order of ``keep``; only a polytope of status OK has rows.  status [n]: OK, THIN (radius <= tol or empty), WHOLE (the whole space) or
    TOO_LARGE; wide [n]: the unbounded or capped runs (their rows were kept); peak [n]: the largest row count a step made; point [n, k]:
    an interior point of the result (OK only).  stats: polytopes, thin, whole, too_large, steps, rows_made, lps, pivots, wide,
    rows_before, rows_after, device_ms, wall_ms."""
    row_off: numpy.ndarray
    rows: numpy.ndarray
    status: numpy.ndarray
    wide: numpy.ndarray
    peak: numpy.ndarray
    point: numpy.ndarray
    stats: dict = field(default_factory=dict)

    def __len__(self) -> int:
        return len(self.status)

    def rows_of(self, q: int) -> numpy.ndarray:
        return self.rows[self.row_off[q]:self.row_off[q + 1]]

    def polytopes(self) -> list:
        """one Polytope per item; an item that is not OK has no rows (read ``status`` to tell the whole space from nothing)"""
        return [Polytope(self.rows_of(q)[:, 1:].copy(), self.rows_of(q)[:, :1].copy()) for q in range(len(self))]


def _columns(who: str, n: int, keep, order):
    """(keep, the columns of the call: the kept ones, then the eliminated ones with the first to go last)"""
    try:
        kept = [int(c) for c in keep]
        same = all(int(c) == c for c in keep)
    except (TypeError, ValueError):
        raise ValueError(f'{who}: keep must be a list of coordinates') from None
    if not kept or not same or len(set(kept)) != len(kept) or min(kept) < 0 or max(kept) >= n:
        raise ValueError(f'{who}: keep must name at least one coordinate of 0..{n - 1}, each once')
    rest = sorted(set(range(n)) - set(kept), reverse=True)
    if order is not None:
        try:
            given = [int(c) for c in order]
        except (TypeError, ValueError):
            raise ValueError(f'{who}: order must be a list of coordinates') from None
        if sorted(given, reverse=True) != rest:
            raise ValueError(f'{who}: order must name the eliminated coordinates {sorted(rest)}, each once')
        rest = given
    return kept, kept + rest[::-1]


def project_rows_of(row_off, rows, n: int, keep, tol: float = 1e-8, start=None, order=None, out_cap: int = MAX_ROWS, device: int = 0,
                    who: str = 'project_rows_of') -> ProjectedRows:
    """The polytopes of unit rows ``rows`` = [o | n] in CSR form by row_off, projected onto the coordinates ``keep`` (the module
    docstring): a ProjectedRows whose rows are in the kept coordinates in the order of ``keep``.  ``order``: the eliminated coordinates
    in the order of their elimination (None: descending index).  ``start``: [polytopes, n] where the first run of each starts (None:
    the origin); any finite point.  ``out_cap``: the most rows a result may have, 1..512.  ValueError before anything reaches the
    device for n outside 1..16, a bad keep or order, a polytope without rows or with more than 512, non-finite or non-unit rows, a
    non-finite start or tol, tol < 0, out_cap outside 1..512."""
    t0 = time.perf_counter()
    off, ef, start = check_rows(who, row_off, rows, n, tol, start)
    kept, cols = _columns(who, n, keep, order)
    if not (isinstance(out_cap, (int, numpy.integer)) and 1 <= out_cap <= MAX_ROWS):
        raise ValueError(f'{who}: out_cap = {out_cap} is outside 1..{MAX_ROWS}')
    from .. import _lib
    cols = numpy.asarray(cols, dtype=numpy.int64)
    lifted = numpy.ascontiguousarray(ef[:, numpy.concatenate([[0], 1 + cols])])
    s0 = None if start is None else numpy.ascontiguousarray(start[:, cols])
    out_off, out, status, wide, peak, point, s = _lib.project_rows(off, lifted, n - len(kept), s0, tol, int(out_cap), device)
    stats = {key: int(s[key]) for key in ('polytopes', 'thin', 'whole', 'too_large', 'steps', 'rows_made', 'lps', 'pivots', 'wide')}
    stats.update(rows_before=int(len(ef)), rows_after=int(len(out)), device_ms=float(s['ms']))
    stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
    return ProjectedRows(row_off=numpy.asarray(out_off, dtype=numpy.int64), rows=numpy.asarray(out, dtype=numpy.float64).reshape(-1, len(kept) + 1),
                         status=numpy.asarray(status, dtype=numpy.int32), wide=numpy.asarray(wide, dtype=numpy.int32),
                         peak=numpy.asarray(peak, dtype=numpy.int32), point=numpy.asarray(point, dtype=numpy.float64), stats=stats)


def _stacked(who: str, plist) -> tuple:
    parts = [polytope_unit_rows(who, p) for p in plist]
    n = parts[0].shape[1] - 1
    if any(q.shape[1] - 1 != n for q in parts):
        raise ValueError(f'{who}: the polytopes have different dimensions')
    off = numpy.concatenate([[0], numpy.cumsum([len(q) for q in parts])]).astype(numpy.int64)
    return off, numpy.vstack(parts), n


def project_polytopes(polytopes: Union[Polytope, Sequence[Polytope]], keep, tol: float = 1e-8, start=None, order=None, out_cap: int = MAX_ROWS,
                      device: int = 0) -> ProjectedRows:
    """project_rows_of for Polytope objects {x : A x <= b}: their rows are scaled to unit normals first (a zero row is a ValueError)."""
    plist = [polytopes] if isinstance(polytopes, Polytope) else list(polytopes)
    if not plist:
        raise ValueError('project_polytopes: no polytopes')
    off, ef, n = _stacked('project_polytopes', plist)
    return project_rows_of(off, ef, n, keep, tol=tol, start=start, order=order, out_cap=out_cap, device=device, who='project_polytopes')


def _one(who: str, r: ProjectedRows) -> Polytope:
    """the only polytope of r: WHOLE has no rows, THIN and TOO_LARGE are ValueErrors"""
    st = int(r.status[0])
    if st in (THIN, TOO_LARGE):
        raise ValueError(f'{who}: the projection is {STATUS[st]} (peak = {int(r.peak[0])} rows)')
    return r.polytopes()[0]


def projected_polytope(p: Polytope, keep, tol: float = 1e-8, device: int = 0) -> Polytope:
    """Polytope.project: see there."""
    rows = polytope_unit_rows('Polytope.project', p)
    r = project_rows_of(numpy.asarray([0, len(rows)], dtype=numpy.int64), rows, rows.shape[1] - 1, keep, tol=tol, device=device, who='Polytope.project')
    return _one('Polytope.project', r)


def affine_image(polytope: Polytope, M, v=None, tol: float = 1e-8, device: int = 0) -> Polytope:
    """{M x + v : x in P} for M [k, n] of full row rank, k <= n.  M is completed to an invertible T = [M; N'] with an orthonormal basis N
    of its null space, P is rewritten in (y, z) = (M x + v, N' x) and z is eliminated on the device.  A square M needs no device.
    ValueError for a rank-deficient M (the image is flat), and for an image that is THIN or TOO_LARGE; the whole space has no rows."""
    who = 'affine_image'
    rows = polytope.rows()
    n = rows.shape[1] - 1
    M = numpy.asarray(M, dtype=numpy.float64)
    if M.ndim != 2 or M.shape[1] != n or not 1 <= M.shape[0] <= n or not numpy.all(numpy.isfinite(M)):
        raise ValueError(f'{who}: M must be a finite [k, {n}] matrix with 1 <= k <= {n}')
    k = M.shape[0]
    v = numpy.zeros(k) if v is None else numpy.asarray(v, dtype=numpy.float64).reshape(-1)
    if v.shape != (k,) or not numpy.all(numpy.isfinite(v)):
        raise ValueError(f'{who}: v must be a finite vector of {k} entries')
    _, sv, Vt = numpy.linalg.svd(M)
    if not sv[k - 1] > max(M.shape) * numpy.finfo(numpy.float64).eps * sv[0]:
        raise ValueError(f'{who}: M has rank below {k}: the image is flat')
    T_inv = numpy.linalg.inv(numpy.vstack([M, Vt[k:]]))
    A = rows[:, 1:] @ T_inv                                   # A x = A T^-1 (y - v, z)
    b = rows[:, 0] + A[:, :k] @ v
    if k == n:
        return Polytope(A, b.reshape(-1, 1))
    lifted = Polytope(A, b.reshape(-1, 1))
    unit = polytope_unit_rows(who, lifted)
    r = project_rows_of(numpy.asarray([0, len(unit)], dtype=numpy.int64), unit, n, list(range(k)), tol=tol, device=device, who=who)
    return _one(who, r)


def minkowski_sum(P: Polytope, Q: Polytope, tol: float = 1e-8, device: int = 0) -> Polytope:
    """{x + y : x in P, y in Q}: the image of P x Q under [I I].  Both in R^n with 2 n <= 16."""
    who = 'minkowski_sum'
    p, q = P.rows(), Q.rows()
    n = p.shape[1] - 1
    if q.shape[1] - 1 != n:
        raise ValueError(f'{who}: the polytopes have different dimensions')
    if 2 * n > MAX_DIM:
        raise ValueError(f'{who}: 2 n = {2 * n} > {MAX_DIM}')
    A = numpy.zeros((len(p) + len(q), 2 * n))
    A[:len(p), :n], A[len(p):, n:] = p[:, 1:], q[:, 1:]
    b = numpy.concatenate([p[:, 0], q[:, 0]]).reshape(-1, 1)
    try:
        return affine_image(Polytope(A, b), numpy.hstack([numpy.eye(n), numpy.eye(n)]), tol=tol, device=device)
    except ValueError as e:
        raise ValueError(str(e).replace('affine_image', who, 1)) from None


def controllable_pre(targets: Union[Polytope, Sequence[Polytope]], A, B, U: Polytope, within: Optional[Polytope] = None, tol: float = 1e-8,
                     out_cap: int = MAX_ROWS, device: int = 0) -> ProjectedRows:
    """For every target C the one-step controllable set {theta : there is u in U with A theta + B u in C}, intersected with ``within``
    if given: the polytope of the rows [c | C_A A, C_A B], [u_b | 0, U_A] (and [w_b | W_A, 0]) in (theta, u), scaled to unit normals,
    with u eliminated.  All targets go in one call; n_theta + n_u <= 16.  A ProjectedRows over theta: a target nothing reaches is THIN,
    one every state reaches is WHOLE."""
    who = 'controllable_pre'
    tlist = [targets] if isinstance(targets, Polytope) else list(targets)
    if not tlist:
        raise ValueError(f'{who}: no targets')
    A = numpy.asarray(A, dtype=numpy.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or not numpy.all(numpy.isfinite(A)):
        raise ValueError(f'{who}: A must be a finite square matrix')
    n_t = A.shape[0]
    B = numpy.asarray(B, dtype=numpy.float64)
    if B.ndim == 1:
        B = B.reshape(-1, 1)                  # one input
    if B.ndim != 2 or B.shape[0] != n_t or not B.shape[1] or not numpy.all(numpy.isfinite(B)):
        raise ValueError(f'{who}: B must be a finite [{n_t}, n_u] matrix')
    n_u = B.shape[1]
    if n_t + n_u > MAX_DIM:
        raise ValueError(f'{who}: n_theta + n_u = {n_t + n_u} > {MAX_DIM}')
    u = U.rows()
    if u.shape[1] - 1 != n_u:
        raise ValueError(f'{who}: U has {u.shape[1] - 1} coordinates, B has {n_u} columns')
    fixed = [numpy.hstack([u[:, :1], numpy.zeros((len(u), n_t)), u[:, 1:]])]
    if within is not None:
        w = within.rows()
        if w.shape[1] - 1 != n_t:
            raise ValueError(f'{who}: within has {w.shape[1] - 1} coordinates, A has {n_t}')
        fixed.append(numpy.hstack([w, numpy.zeros((len(w), n_u))]))
    lifted = []
    for C in tlist:
        c = C.rows()
        if c.shape[1] - 1 != n_t:
            raise ValueError(f'{who}: a target has {c.shape[1] - 1} coordinates, A has {n_t}')
        rows = numpy.vstack([numpy.hstack([c[:, :1], c[:, 1:] @ A, c[:, 1:] @ B])] + fixed)
        lifted.append(Polytope(rows[:, 1:], rows[:, :1]))
    off, ef, n = _stacked(who, lifted)
    return project_rows_of(off, ef, n, list(range(n_t)), tol=tol, out_cap=out_cap, device=device, who=who)
