"""Removing the redundant rows of polytopes on the device.

A polytope P is given as unit rows [o | n] (|n| = 1, {theta : n.theta <= o}), m rows in order; ``tol`` has the meaning of §3.19 to §3.21:
a set whose Chebyshev radius is not above tol does not count.

  thin             radius(P) <= tol: P is THIN.  It is returned unchanged and no row is tested.
  sequential rule  otherwise, for k = 0 .. m - 1 in order, let L be the rows still live: the rows before k that were kept and all rows
                   after k.  Row k is redundant iff the radius run over L n {n_k.theta >= o_k} (L and row k reversed) ends optimal with
                   t <= tol.  A redundant row is removed at once and is not in L for later rows.
  safe direction   a run that is unbounded or stopped at the pivot cap counts as "kept" and the polytope is flagged wide: the reduced
                   polytope never loses a state of P.

What follows from the rule: of exact duplicates the last one survives (the first is redundant against the second, which is still live);
a row that touches P only in a lower-dimensional face is removed; the result contains P, and every removed row cut off a set of radius
<= tol at the time of its removal; the result is deterministic and depends on the row order.  Every LP runs on the device
(csrc/reduce.hpp, k_reduce_rows, one wavefront per polytope), up to 512 rows per polytope and n_theta <= 16.
"""
import time
from dataclasses import dataclass, field
from typing import Sequence, Union

import numpy

from .._pairs import MAX_DIM, check_region_limits, check_rows_finite, check_scalars
from .polytope import Polytope

__all__ = ['ReducedRows', 'reduce_rows_of', 'reduce_polytopes', 'MAX_ROWS', 'MAX_DIM', 'OK', 'THIN']

MAX_ROWS = 512    # RD_MAX_ROWS of csrc/reduce.hpp
OK, THIN = 0, 1   # status of a polytope (MPC_REDUCE_OK, MPC_REDUCE_THIN)


@dataclass
class ReducedRows:
    """The reduced polytopes in CSR form: polytope q keeps rows[row_off[q]:row_off[q + 1]], its kept rows in the original order with
    their bits unchanged.  kept: one bool per input row; status [n]: OK or THIN (unchanged); wide [n]: the unbounded or capped runs
    (their rows were kept); point [n, n_t]: where the first run ended, interior for a polytope that is neither thin nor wide.
    stats: polytopes, thin, lps, pivots, wide, rows_before, rows_after, device_ms, wall_ms."""
    row_off: numpy.ndarray
    rows: numpy.ndarray
    kept: numpy.ndarray
    status: numpy.ndarray
    wide: numpy.ndarray
    point: numpy.ndarray
    stats: dict = field(default_factory=dict)

    def __len__(self) -> int:
        return len(self.status)

    def rows_of(self, q: int) -> numpy.ndarray:
        return self.rows[self.row_off[q]:self.row_off[q + 1]]

    def polytopes(self) -> list:
        return [Polytope(self.rows_of(q)[:, 1:].copy(), self.rows_of(q)[:, :1].copy()) for q in range(len(self))]


def check_rows(who: str, row_off, ef_rows, n_t: int, tol: float, start=None):
    """(off int64, ef float64 [rows, n_t + 1], start or None) of a call the device accepts; ValueError in the name of ``who`` otherwise."""
    check_scalars(who, n_t, tol)
    off = numpy.ascontiguousarray(row_off, dtype=numpy.int64).reshape(-1)
    ef = numpy.asarray(ef_rows, dtype=numpy.float64)
    if ef.ndim != 2 or ef.shape[1] != n_t + 1:
        raise ValueError(f'{who}: ef_rows must be [rows, {n_t + 1}], not {list(ef.shape)}')
    ef = numpy.ascontiguousarray(ef)
    if len(off) < 2 or off[0] != 0 or off[-1] != len(ef):
        raise ValueError(f'{who}: row_off [n + 1] must run from 0 to the number of rows and describe n >= 1 polytopes')
    check_rows_finite(who, off, [ef], MAX_ROWS)
    if numpy.any(numpy.abs(numpy.sqrt(numpy.sum(ef[:, 1:] * ef[:, 1:], axis=1)) - 1.0) > 1e-6):
        raise ValueError(f'{who}: rows must have unit normals')
    if start is not None:
        start = numpy.ascontiguousarray(start, dtype=numpy.float64)
        if start.shape != (len(off) - 1, n_t) or not numpy.all(numpy.isfinite(start)):
            raise ValueError(f'{who}: start must be a finite [{len(off) - 1}, {n_t}] array')
    return off, ef, start


def reduce_rows_of(row_off, ef_rows, n_t: int, tol: float = 1e-8, start=None, device: int = 0, who: str = 'reduce_rows_of') -> ReducedRows:
    """The polytopes of unit rows ef_rows = [o | n] in CSR form by row_off without their redundant rows (the module docstring): a
    ReducedRows.  ``start``: [n, n_t] where the first run of each polytope starts (None: the origin); any finite point.  ValueError before
    anything reaches the device for n_t outside 1..16, a polytope without rows or with more than 512, non-finite or non-unit rows, a
    non-finite start or tol, tol < 0."""
    from .. import _lib
    t0 = time.perf_counter()
    off, ef, start = check_rows(who, row_off, ef_rows, n_t, tol, start)
    kept, status, wide, point, s = _lib.reduce_rows(off, ef, start, tol, device)
    kept = numpy.asarray(kept, dtype=bool).reshape(-1)
    new_off = numpy.concatenate([[0], numpy.cumsum(numpy.add.reduceat(kept.astype(numpy.int64), off[:-1]))]).astype(numpy.int64)
    stats = {'polytopes': int(s['polytopes']), 'thin': int(s['thin']), 'lps': int(s['lps']), 'pivots': int(s['pivots']), 'wide': int(s['wide']),
             'rows_before': int(len(ef)), 'rows_after': int(kept.sum()), 'device_ms': float(s['ms'])}
    stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
    return ReducedRows(row_off=new_off, rows=ef[kept], kept=kept, status=numpy.asarray(status, dtype=numpy.int32),
                       wide=numpy.asarray(wide, dtype=numpy.int32), point=numpy.asarray(point, dtype=numpy.float64), stats=stats)


def polytope_unit_rows(who: str, p: Polytope) -> numpy.ndarray:
    """[m, n + 1] unit rows [o | n] of {A x <= b}; ValueError for a row without a normal"""
    rows = p.rows()
    nrm = numpy.linalg.norm(rows[:, 1:], axis=1)
    if not len(rows) or numpy.any(~(nrm > 0.0)):
        raise ValueError(f'{who}: a polytope has no rows, or a row without a normal (a zero row)')
    return rows / nrm[:, None]


def reduce_polytopes(polytopes: Union[Polytope, Sequence[Polytope]], tol: float = 1e-8, start=None, device: int = 0) -> ReducedRows:
    """reduce_rows_of for Polytope objects {x : A x <= b}: their rows are scaled to unit normals first (a zero row is a ValueError), so
    ``rows`` of the result holds unit rows and ``kept`` indexes the rows of each A in order."""
    plist = [polytopes] if isinstance(polytopes, Polytope) else list(polytopes)
    if not plist:
        raise ValueError('reduce_polytopes: no polytopes')
    parts = [polytope_unit_rows('reduce_polytopes', p) for p in plist]
    n = parts[0].shape[1] - 1
    if any(q.shape[1] - 1 != n for q in parts):
        raise ValueError('reduce_polytopes: the polytopes have different dimensions')
    off = numpy.concatenate([[0], numpy.cumsum([len(q) for q in parts])]).astype(numpy.int64)
    return reduce_rows_of(off, numpy.vstack(parts), n, tol=tol, start=start, device=device, who='reduce_polytopes')


def reduced_polytope(p: Polytope, tol: float = 1e-8, device: int = 0) -> Polytope:
    """Polytope.reduced: the rows of p the sequential rule keeps, as they are in p (unscaled)."""
    rows = polytope_unit_rows('Polytope.reduced', p)
    n = rows.shape[1] - 1
    r = reduce_rows_of(numpy.asarray([0, len(rows)], dtype=numpy.int64), rows, n, tol=tol, device=device, who='Polytope.reduced')
    A, b = numpy.asarray(p.A, dtype=numpy.float64), numpy.asarray(p.b, dtype=numpy.float64).reshape(len(rows), -1)
    return Polytope(A[r.kept].copy(), b[r.kept].copy())


def reduce_solution(source, tol: float = 1e-8, device: int = 0):
    """Solution.reduce_rows: see there.  Rows of E without a normal take no part (they stay where they are); a region such a row empties
    is copied unchanged."""
    import copy
    from ..solution import Solution
    who = 'reduce_rows'
    regs = source.critical_regions
    if not regs:
        raise ValueError(f'{who}: the solution has no regions')
    if source.merge_info is None and source.overlap_info is None:
        raise ValueError(f'{who}: only the results of merge_regions and remove_overlaps are reduced (their regions own their E, f)')
    n_t = source.theta_dim() if source.program is not None else numpy.asarray(regs[0].E).shape[1]
    check_region_limits(who, (), n_t)
    if not (numpy.isfinite(tol) and tol >= 0.0):
        raise ValueError(f'{who}: tol must be finite and >= 0')
    parts, index, void = [], [], []
    for i, r in enumerate(regs):
        E = numpy.asarray(r.E, dtype=numpy.float64).reshape(-1, n_t)
        f = numpy.asarray(r.f, dtype=numpy.float64).reshape(-1)
        nrm = numpy.linalg.norm(E, axis=1)
        idx = numpy.flatnonzero(nrm > 0.0)
        if not len(idx):
            raise ValueError(f'{who}: region {i} has no row with a normal (the whole space, or nothing)')
        if len(idx) > MAX_ROWS:
            raise ValueError(f'{who}: region {i} has more than {MAX_ROWS} rows')
        void.append(bool(numpy.any((nrm == 0.0) & (f < 0.0))))
        index.append(idx)
        parts.append(numpy.hstack([(f[idx] / nrm[idx]).reshape(-1, 1), E[idx] / nrm[idx, None]]))
    off = numpy.concatenate([[0], numpy.cumsum([len(q) for q in parts])]).astype(numpy.int64)
    red = reduce_rows_of(off, numpy.vstack(parts), n_t, tol=tol, device=device, who=who)
    out = []
    for i, r in enumerate(regs):
        q = copy.copy(r)
        E = numpy.asarray(r.E, dtype=numpy.float64).reshape(-1, n_t)
        f = numpy.asarray(r.f, dtype=numpy.float64).reshape(len(E), -1)
        keep = numpy.ones(len(E), dtype=bool)
        if not void[i]:
            keep[index[i]] = red.kept[off[i]:off[i + 1]]
        q.E, q.f = E[keep].copy(), f[keep].copy()
        out.append(q)
    sol = Solution(source.program, out, is_overlapping=source.is_overlapping, point_location_tolerance=source.point_location_tolerance)
    sol.is_complete = source.is_complete
    sol.merge_info, sol.overlap_info = source.merge_info, source.overlap_info
    sol.reduce_info = {'source': source, 'kept': red.kept, 'row_off': off, 'status': red.status, 'wide': red.wide, 'stats': dict(red.stats)}
    return sol
