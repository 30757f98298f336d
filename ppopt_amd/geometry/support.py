"""Support functions of polytopes on the device: Pontryagin differences, containment, ranges of the control law.

A polytope P of R^n is given as unit rows [o | n] (|n| = 1, {x : n.x <= o}); h_P(d) = max {d.x : x in P} is its support function.
``tol`` has the meaning of §3.19 to §3.27: a set whose Chebyshev radius is not above tol does not count.

  interior point  the radius run over the rows from the start point (the origin without one), stopped once t > tol.  Optimal with
                  t <= tol: P is THIN, every direction gets value = arg = NaN and the status THIN.  Otherwise the point p where the run
                  ended.  An unbounded or capped radius run is not thin and is flagged in ``wide``: an unbounded run, which ends while
                  t <= tol and need not have reached P, moves p along the ray it found to t = tol + 1, a point of P of that radius; a
                  capped run with t >= 0 goes on from the point reached; a capped run with t < 0 knows no point of P and every direction
                  gets value +inf, arg NaN and CAPPED.
  one direction   d = 0: value 0, arg p, no LP.  Otherwise the vertex simplex maximises (d / |d|).x from p with a fresh basis.  Optimal:
                  arg is the point reached and value = d.arg.  UNBOUNDED: value +inf.  CAPPED (the pivot cap): value +inf, a bound and
                  not a value.
  independence    every run starts from p alone: the result of a direction depends on (rows, start, tol, d) only.  Permuting a list,
                  repeating a direction or sending each distinct direction once changes no bit of any result.

What is built on it: P - Q = {x : x + q in P for every q in Q} = {x : n_k.x <= o_k - h_Q(n_k)} (pontryagin_difference), P in Q iff
h_P(n_k) <= o_k for every row of Q (containment), and the smallest and largest value of every row of the control law over every region
(Solution.output_range).  Every LP runs on the device (csrc/support.hpp, k_support_rows, one wavefront per block of directions of one
polytope): n <= 16, at most 512 rows per polytope, full-dimensional polytopes only.
"""
import time
from dataclasses import dataclass, field
from typing import Optional, Sequence, Union

import numpy

from .polytope import Polytope
from .reduce import check_rows, polytope_unit_rows

__all__ = ['SupportValues', 'ErodedRows', 'Containment', 'OutputRange', 'support_of', 'support', 'pontryagin_difference', 'containment',
           'robust_controllable_pre', 'output_range', 'MAX_ROWS', 'MAX_DIM', 'OK', 'UNBOUNDED', 'CAPPED', 'THIN', 'STATUS', 'ERODED_OK',
           'ERODED_EMPTY', 'ERODED_THIN', 'ERODED_STATUS']

MAX_ROWS = 512    # SF_MAX_ROWS of csrc/support.hpp
MAX_DIM = 16
OK, UNBOUNDED, CAPPED, THIN = range(4)   # status of a direction (MPC_SUPPORT_*); a polytope is OK or THIN
STATUS = ('OK', 'UNBOUNDED', 'CAPPED', 'THIN')
ERODED_OK, ERODED_EMPTY, ERODED_THIN = range(3)   # status of a Pontryagin difference
ERODED_STATUS = ('OK', 'EMPTY', 'THIN')


@dataclass
class SupportValues:
    """h_P(d) of every polytope and each of its directions: polytope q owns the entries dir_off[q]:dir_off[q + 1].  value [n_dir]: the
    support value, +inf for UNBOUNDED and CAPPED, NaN for THIN; arg [n_dir, n] (None without ``args``): a point of P that attains it (the
    last point reached where the value is +inf); dir_status [n_dir]: OK, UNBOUNDED, CAPPED or THIN; poly_status [n_poly]: OK or THIN;
    wide [n_poly]: 1 where the radius run was unbounded or capped; point [n_poly, n]: where the radius run ended, the start of every
    direction.  stats: polytopes, thin, directions, zero, lps, pivots, wide, device_ms, wall_ms."""
    dir_off: numpy.ndarray
    value: numpy.ndarray
    arg: Optional[numpy.ndarray]
    dir_status: numpy.ndarray
    poly_status: numpy.ndarray
    wide: numpy.ndarray
    point: numpy.ndarray
    stats: dict = field(default_factory=dict)

    def __len__(self) -> int:
        return len(self.poly_status)

    def values_of(self, q: int) -> numpy.ndarray:
        return self.value[self.dir_off[q]:self.dir_off[q + 1]]

    def args_of(self, q: int) -> numpy.ndarray:
        return self.arg[self.dir_off[q]:self.dir_off[q + 1]]


def check_directions(who: str, dir_off, dirs, n_poly: int, n: int):
    """(dir_off int64 [n_poly + 1], dirs float64 [n_dir, n]) of a call the device accepts; ValueError in the name of ``who`` otherwise."""
    doff = numpy.ascontiguousarray(dir_off, dtype=numpy.int64).reshape(-1)
    d = numpy.asarray(dirs, dtype=numpy.float64)
    if d.ndim != 2 or d.shape[1] != n:
        raise ValueError(f'{who}: dirs must be [directions, {n}], not {list(d.shape)}')
    d = numpy.ascontiguousarray(d)
    if len(doff) != n_poly + 1 or doff[0] != 0 or doff[-1] != len(d) or numpy.any(numpy.diff(doff) < 0):
        raise ValueError(f'{who}: dir_off [{n_poly + 1}] must run from 0 to the number of directions without decreasing')
    if len(d) > 0x7fffffff:
        raise ValueError(f'{who}: more than 2^31 - 1 directions')
    if not numpy.all(numpy.isfinite(d)):
        raise ValueError(f'{who}: directions must be finite')
    return doff, d


def support_of(row_off, rows, n: int, dir_off, dirs, tol: float = 1e-8, start=None, args: bool = True, device: int = 0,
               who: str = 'support_of') -> SupportValues:
    """h_P(d) for the polytopes of unit rows ``rows`` = [o | n] in CSR form by row_off and their directions dirs [n_dir, n] in CSR form by
    dir_off (the module docstring): a SupportValues.  ``start``: [polytopes, n] where the radius run of each starts (None: the origin); any
    finite point.  ``args``: return the maximisers.  ValueError before anything reaches the device for n outside 1..16, a polytope
    without rows or with more than 512, non-finite or non-unit rows, a dir_off that does not run from 0 to the number of directions, a
    non-finite direction, start or tol, tol < 0."""
    t0 = time.perf_counter()
    off, ef, start = check_rows(who, row_off, rows, n, tol, start)
    doff, d = check_directions(who, dir_off, dirs, len(off) - 1, n)
    from .. import _lib
    value, arg, ds, ps, wide, point, s = _lib.support_rows(off, ef, doff, d, start, tol, args=bool(args), device=device)
    stats = {key: int(s[key]) for key in ('polytopes', 'thin', 'directions', 'zero', 'lps', 'pivots', 'wide')}
    stats['device_ms'] = float(s['ms'])
    stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
    return SupportValues(dir_off=doff, value=numpy.asarray(value, dtype=numpy.float64),
                         arg=None if arg is None else numpy.asarray(arg, dtype=numpy.float64).reshape(-1, n),
                         dir_status=numpy.asarray(ds, dtype=numpy.int32), poly_status=numpy.asarray(ps, dtype=numpy.int32),
                         wide=numpy.asarray(wide, dtype=numpy.int32), point=numpy.asarray(point, dtype=numpy.float64).reshape(-1, n), stats=stats)


def _stacked(who: str, plist) -> tuple:
    """(row_off, unit rows, n) of Polytope objects"""
    parts = [polytope_unit_rows(who, p) for p in plist]
    n = parts[0].shape[1] - 1
    if any(q.shape[1] - 1 != n for q in parts):
        raise ValueError(f'{who}: the polytopes have different dimensions')
    off = numpy.concatenate([[0], numpy.cumsum([len(q) for q in parts])]).astype(numpy.int64)
    return off, numpy.vstack(parts), n


def _plist(who: str, polytopes, what: str = 'polytopes') -> list:
    plist = [polytopes] if isinstance(polytopes, Polytope) else list(polytopes)
    if not plist:
        raise ValueError(f'{who}: no {what}')
    return plist


def _direction_table(who: str, directions, n_poly: int, n: int):
    """(dir_off, dirs) of one [k, n] array for all polytopes, or of a list with one array per polytope"""
    if isinstance(directions, (list, tuple)) and len(directions) and all(numpy.ndim(d) == 2 for d in directions):
        parts = [numpy.asarray(d, dtype=numpy.float64) for d in directions]
        if len(parts) != n_poly:
            raise ValueError(f'{who}: {len(parts)} direction lists for {n_poly} polytopes')
    else:
        one = numpy.asarray(directions, dtype=numpy.float64)
        parts = [one.reshape(1, n) if one.ndim == 1 and one.size == n else one] * n_poly
    parts = [p.reshape(0, n) if p.size == 0 else p for p in parts]
    if any(p.ndim != 2 or p.shape[1] != n for p in parts):
        raise ValueError(f'{who}: directions must be [k, {n}] arrays')
    off = numpy.concatenate([[0], numpy.cumsum([len(p) for p in parts])]).astype(numpy.int64)
    return off, numpy.vstack(parts) if parts else numpy.zeros((0, n))


def support(polytopes: Union[Polytope, Sequence[Polytope]], directions, tol: float = 1e-8, start=None, args: bool = True,
            device: int = 0) -> SupportValues:
    """support_of for Polytope objects {x : A x <= b}: their rows are scaled to unit normals first (a zero row is a ValueError).
    ``directions``: one [k, n] array used for every polytope, or a list with one array per polytope.  The values are those of the
    directions as given, whatever their length."""
    who = 'support'
    plist = _plist(who, polytopes)
    off, ef, n = _stacked(who, plist)
    doff, d = _direction_table(who, directions, len(plist), n)
    return support_of(off, ef, n, doff, d, tol=tol, start=start, args=args, device=device, who=who)


def polytope_support(p: Polytope, directions, tol: float = 1e-8, device: int = 0):
    """Polytope.support: see there."""
    who = 'Polytope.support'
    rows = polytope_unit_rows(who, p)
    n = rows.shape[1] - 1
    d = numpy.asarray(directions, dtype=numpy.float64)
    single = d.ndim == 1
    if d.ndim not in (1, 2) or (d.size and d.shape[-1] != n) or (single and not d.size):
        raise ValueError(f'{who}: directions must be one direction [{n}] or an array [k, {n}], not {list(d.shape)}')
    d = d.reshape(-1, n)
    r = support_of(numpy.asarray([0, len(rows)], dtype=numpy.int64), rows, n, numpy.asarray([0, len(d)], dtype=numpy.int64), d, tol=tol,
                   device=device, who=who)
    return (r.value[0], r.arg[0]) if single else (r.value, r.arg)


# ---- Pontryagin difference --------------------------------------------------------------------------------------------------------------
@dataclass
class ErodedRows:
    """The differences P - E Q in CSR form: polytope q has rows[row_off[q]:row_off[q + 1]], rows [o_k - h_k | n_k] whose normals are the
    bytes of P's unit rows; only a polytope of status ERODED_OK has rows.  status [n]: ERODED_OK, ERODED_EMPTY (some h_k = +inf: Q is
    unbounded, or a run was capped, in a direction P bounds) or ERODED_THIN (the reduce found a radius <= tol); wide [n]: the unbounded or
    capped runs of its directions, of the radius run of its Q and of its reduce; support: h_k for every row of every P in input order (in_off [n + 1] are the
    offsets).  stats: those of the support call (directions: the distinct ones that were sent), rows_before, rows_after, and with
    reduce_rows reduce_lps, reduce_pivots; device_ms, wall_ms."""
    row_off: numpy.ndarray
    rows: numpy.ndarray
    status: numpy.ndarray
    wide: numpy.ndarray
    support: numpy.ndarray
    in_off: numpy.ndarray
    stats: dict = field(default_factory=dict)

    def __len__(self) -> int:
        return len(self.status)

    def rows_of(self, q: int) -> numpy.ndarray:
        return self.rows[self.row_off[q]:self.row_off[q + 1]]

    def polytopes(self) -> list:
        """one Polytope per item; an item that is not ERODED_OK has no rows (read ``status``)"""
        return [Polytope(self.rows_of(q)[:, 1:].copy(), self.rows_of(q)[:, :1].copy()) for q in range(len(self))]


def _distinct_rows(d: numpy.ndarray):
    """(the distinct rows of d by their bytes, inverse): d == distinct[inverse] bit for bit"""
    d = numpy.ascontiguousarray(d)
    if not len(d):
        return d, numpy.zeros(0, dtype=numpy.int64)
    keys = d.view(numpy.dtype((numpy.void, d.dtype.itemsize * d.shape[1]))).reshape(-1)
    _, first, inverse = numpy.unique(keys, return_index=True, return_inverse=True)
    return d[first], numpy.asarray(inverse, dtype=numpy.int64).reshape(-1)


def pontryagin_difference(P: Union[Polytope, Sequence[Polytope]], Q: Union[Polytope, Sequence[Polytope]], E=None, tol: float = 1e-8,
                          reduce_rows: bool = True, device: int = 0, who: str = 'pontryagin_difference') -> ErodedRows:
    """P - E Q = {x : x + E q in P for every q in Q} for every P: the rows [o_k - h_Q(E' n_k) | n_k] over the unit rows [o_k | n_k] of P.
    Q is one polytope shared by every P (its distinct directions are then sent once and scattered back, which independence makes exact)
    or a list with one Q per P.  ``E``: [n, n_q] (None: the identity, Q in the space of P); Q lives in its own space and must be
    full-dimensional there: a thin Q is a ValueError.  ``reduce_rows``: the rows go through reduce_rows_of started from the origin, the
    kept rows come back in order with their bits unchanged and a radius <= tol is ERODED_THIN; without it the raw rows come back and a
    difference that is empty is not detected."""
    t0 = time.perf_counter()
    plist = _plist(who, P)
    shared = isinstance(Q, Polytope)
    qlist = [Q] if shared else list(Q)
    if not shared and len(qlist) != len(plist):
        raise ValueError(f'{who}: {len(qlist)} polytopes Q for {len(plist)} polytopes P')
    off, ef, n = _stacked(who, plist)
    qoff, qef, n_q = _stacked(who, qlist)
    if E is None:
        if n_q != n:
            raise ValueError(f'{who}: Q has {n_q} coordinates, P has {n}: give E [{n}, {n_q}]')
        dirs = numpy.ascontiguousarray(ef[:, 1:])
    else:
        E = numpy.asarray(E, dtype=numpy.float64)
        if E.shape != (n, n_q) or not numpy.all(numpy.isfinite(E)):
            raise ValueError(f'{who}: E must be a finite [{n}, {n_q}] matrix')
        dirs = numpy.ascontiguousarray(ef[:, 1:] @ E)         # E' n_k, one row per row of P
    check_rows(who, off, ef, n, tol)
    if shared:
        sent, inverse = _distinct_rows(dirs)
        doff = numpy.asarray([0, len(sent)], dtype=numpy.int64)
    else:
        sent, inverse, doff = dirs, numpy.arange(len(dirs)), off
    sv = support_of(qoff, qef, n_q, doff, sent, tol=tol, args=False, device=device, who=who)
    if numpy.any(sv.poly_status == THIN):
        raise ValueError(f'{who}: Q is THIN (Chebyshev radius <= tol): it must be full-dimensional in its own space')
    h = sv.value[inverse]
    run_wide = (sv.dir_status[inverse] != OK).astype(numpy.int64)
    n_poly = len(plist)
    wide = numpy.add.reduceat(run_wide, off[:-1]).astype(numpy.int32)
    status = numpy.where(wide > 0, ERODED_EMPTY, ERODED_OK).astype(numpy.int32)
    wide += sv.wide[0] if shared else sv.wide              # the radius run of its Q was unbounded or capped
    counts = numpy.diff(off)
    live = numpy.repeat(status == ERODED_OK, counts)
    raw = ef[live].copy()
    raw[:, 0] = ef[live, 0] - h[live]
    out_counts = numpy.where(status == ERODED_OK, counts, 0)
    stats = dict(sv.stats)
    stats['rows_before'] = int(len(ef))
    if reduce_rows and len(raw):
        from .reduce import THIN as RD_THIN, reduce_rows_of
        ok = numpy.flatnonzero(status == ERODED_OK)
        roff = numpy.concatenate([[0], numpy.cumsum(out_counts[ok])]).astype(numpy.int64)
        red = reduce_rows_of(roff, raw, n, tol=tol, device=device, who=who)
        thin = red.status == RD_THIN
        status[ok[thin]] = ERODED_THIN
        wide[ok] += red.wide
        keep = red.kept & ~numpy.repeat(thin, numpy.diff(roff))
        raw = raw[keep]
        out_counts[ok] = numpy.add.reduceat(keep.astype(numpy.int64), roff[:-1])
        stats.update(reduce_lps=int(red.stats['lps']), reduce_pivots=int(red.stats['pivots']))
        stats['device_ms'] += float(red.stats['device_ms'])
    stats['rows_after'] = int(len(raw))
    stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
    row_off = numpy.concatenate([[0], numpy.cumsum(out_counts)]).astype(numpy.int64)
    assert len(status) == n_poly and row_off[-1] == len(raw)
    return ErodedRows(row_off=row_off, rows=raw, status=status, wide=wide, support=h, in_off=off, stats=stats)


def eroded_polytope(p: Polytope, Q: Polytope, E=None, tol: float = 1e-8, reduce_rows: bool = True, device: int = 0) -> Polytope:
    """Polytope.erode: see there."""
    who = 'Polytope.erode'
    r = pontryagin_difference(p, Q, E=E, tol=tol, reduce_rows=reduce_rows, device=device, who=who)
    st = int(r.status[0])
    if st != ERODED_OK:
        raise ValueError(f'{who}: the difference is {ERODED_STATUS[st]}')
    return r.polytopes()[0]


# ---- containment ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Containment:
    """For every pair (i, j): excess = max_k (h_{P_i}(n_k) - o_k) over the unit rows [o_k | n_k] of outer polytope j, the lowest row k
    that attains it, the point of P_i that does (``witness``) and inside = excess <= tol.  An unbounded or capped run gives excess =
    +inf, a thin inner polytope NaN (row -1); both are not inside.  stats: those of the support call."""
    pairs: numpy.ndarray
    excess: numpy.ndarray
    row: numpy.ndarray
    witness: numpy.ndarray
    inside: numpy.ndarray
    stats: dict = field(default_factory=dict)

    def __len__(self) -> int:
        return len(self.excess)


def containment(inner: Union[Polytope, Sequence[Polytope]], outer: Union[Polytope, Sequence[Polytope]], pairs=None, tol: float = 1e-8,
                device: int = 0, who: str = 'containment') -> Containment:
    """Is inner polytope i a subset of outer polytope j, for every pair (i, j) of ``pairs`` (None: the two lists element by element):
    a Containment.  The direction list of inner polytope i is the concatenation of the normals of its partners' rows, in pair order."""
    ilist, olist = _plist(who, inner, 'inner polytopes'), _plist(who, outer, 'outer polytopes')
    off, ef, n = _stacked(who, ilist)
    ooff, oef, n_o = _stacked(who, olist)
    if n_o != n:
        raise ValueError(f'{who}: the inner polytopes have {n} coordinates, the outer ones {n_o}')
    if pairs is None:
        if len(ilist) != len(olist):
            raise ValueError(f'{who}: {len(ilist)} inner and {len(olist)} outer polytopes: name the pairs')
        pr = numpy.stack([numpy.arange(len(ilist)), numpy.arange(len(ilist))], axis=1).astype(numpy.int64)
    else:
        pr = numpy.asarray(pairs)
        if pr.size == 0 or pr.ndim != 2 or pr.shape[1] != 2 or not numpy.issubdtype(pr.dtype, numpy.integer):
            raise ValueError(f'{who}: pairs must be a non-empty [k, 2] list of integer pairs (inner, outer)')
        pr = pr.astype(numpy.int64)
        if pr.min() < 0 or pr[:, 0].max() >= len(ilist) or pr[:, 1].max() >= len(olist):
            raise ValueError(f'{who}: a pair names a polytope out of range')
    order = numpy.argsort(pr[:, 0], kind='stable')            # the pairs grouped by inner polytope, in pair order inside a group
    m_outer = numpy.diff(ooff)
    per_pair = m_outer[pr[order, 1]]
    per_inner = numpy.zeros(len(ilist), dtype=numpy.int64)
    numpy.add.at(per_inner, pr[order, 0], per_pair)
    doff = numpy.concatenate([[0], numpy.cumsum(per_inner)]).astype(numpy.int64)
    pair_off = numpy.concatenate([[0], numpy.cumsum(per_pair)]).astype(numpy.int64)     # inner ascending: the table's own order
    take = numpy.concatenate([numpy.arange(ooff[j], ooff[j + 1]) for j in pr[order, 1]])
    sv = support_of(off, ef, n, doff, oef[take, 1:], tol=tol, device=device, who=who)
    np_ = len(pr)
    excess, row, witness = numpy.full(np_, numpy.nan), numpy.full(np_, -1, dtype=numpy.int64), numpy.full((np_, n), numpy.nan)
    gap = sv.value - oef[take, 0]
    for s, p in enumerate(order):
        g = gap[pair_off[s]:pair_off[s + 1]]
        if numpy.any(numpy.isnan(g)):
            continue
        k = int(numpy.argmax(g))
        excess[p], row[p], witness[p] = g[k], k, sv.arg[pair_off[s] + k]
    return Containment(pairs=pr, excess=excess, row=row, witness=witness, inside=excess <= tol, stats=dict(sv.stats))


def polytope_contains(p: Polytope, other: Polytope, tol: float = 1e-8, device: int = 0) -> bool:
    """Polytope.contains_polytope: see there."""
    return bool(containment(other, p, tol=tol, device=device, who='Polytope.contains_polytope').inside[0])


# ---- robust one-step controllable sets --------------------------------------------------------------------------------------------------
def robust_controllable_pre(targets: Union[Polytope, Sequence[Polytope]], A, B, U: Polytope, W: Polytope, E=None,
                            within: Optional[Polytope] = None, tol: float = 1e-8, out_cap: int = MAX_ROWS, device: int = 0):
    """For every target C the states theta with some u in U such that A theta + B u + E w lies in C for every disturbance w in W:
    controllable_pre of pontryagin_difference(targets, W, E).  A ProjectedRows over theta with one entry per target; a target whose
    difference is EMPTY or THIN gives what controllable_pre gives for a target nothing reaches (THIN, no rows)."""
    from . import project
    who = 'robust_controllable_pre'
    tlist = _plist(who, targets, 'targets')
    er = pontryagin_difference(tlist, W, E=E, tol=tol, reduce_rows=True, device=device, who=who)
    ok = numpy.flatnonzero(er.status == ERODED_OK)
    n_t = numpy.asarray(A).shape[0] if numpy.ndim(A) == 2 else 0
    eroded = er.polytopes()
    if not len(ok):
        n_all = len(tlist)
        return project.ProjectedRows(row_off=numpy.zeros(n_all + 1, dtype=numpy.int64), rows=numpy.zeros((0, n_t + 1)),
                                     status=numpy.full(n_all, project.THIN, dtype=numpy.int32), wide=numpy.zeros(n_all, dtype=numpy.int32),
                                     peak=numpy.zeros(n_all, dtype=numpy.int32), point=numpy.zeros((n_all, n_t)),
                                     stats={'erosion': dict(er.stats)})
    pre = project.controllable_pre([eroded[q] for q in ok], A, B, U, within=within, tol=tol, out_cap=out_cap, device=device)
    n_all = len(tlist)
    status = numpy.full(n_all, project.THIN, dtype=numpy.int32)
    wide, peak = numpy.zeros(n_all, dtype=numpy.int32), numpy.zeros(n_all, dtype=numpy.int32)
    point, counts = numpy.zeros((n_all, pre.point.shape[1])), numpy.zeros(n_all, dtype=numpy.int64)
    status[ok], wide[ok], peak[ok], point[ok], counts[ok] = pre.status, pre.wide, pre.peak, pre.point, numpy.diff(pre.row_off)
    stats = dict(pre.stats)
    stats['erosion'] = dict(er.stats)
    return project.ProjectedRows(row_off=numpy.concatenate([[0], numpy.cumsum(counts)]).astype(numpy.int64), rows=pre.rows, status=status,
                                 wide=wide, peak=peak, point=point, stats=stats)


# ---- the range of the control law over the regions of a solution --------------------------------------------------------------------------
@dataclass
class OutputRange:
    """lo [R, K], hi [R, K]: the smallest and largest value of law row outputs[k] over region i; arg_lo, arg_hi [R, K, n_theta]: where
    they are attained; flag [R, K]: a run was unbounded or capped, the entry is a bound (-inf or +inf) and not a value; thin [R]: the
    region's Chebyshev radius is <= tol, its entries are NaN.  stats: those of the support call."""
    outputs: list
    lo: numpy.ndarray
    hi: numpy.ndarray
    arg_lo: numpy.ndarray
    arg_hi: numpy.ndarray
    flag: numpy.ndarray
    thin: numpy.ndarray
    stats: dict = field(default_factory=dict)

    def overall(self):
        """(lo [K], hi [K], region [K, 2], theta [K, 2, n_theta]) over all regions that are not thin: the extremes of every row, the
        regions (lowest index first) that attain the minimum and the maximum, and the points where they do"""
        K = self.lo.shape[1]
        use = numpy.flatnonzero(~self.thin)
        if not len(use):
            raise ValueError('OutputRange.overall: every region is thin')
        i_lo, i_hi = use[numpy.argmin(self.lo[use], axis=0)], use[numpy.argmax(self.hi[use], axis=0)]
        k = numpy.arange(K)
        return (self.lo[i_lo, k], self.hi[i_hi, k], numpy.stack([i_lo, i_hi], axis=1),
                numpy.stack([self.arg_lo[i_lo, k], self.arg_hi[i_hi, k]], axis=1))


def output_range(solution, outputs=None, tol: float = 1e-8, device: int = 0) -> OutputRange:
    """Solution.output_range: see there."""
    from ..compare import _laws, _n_theta, output_rows
    who = 'output_range'
    if not solution.critical_regions:
        raise ValueError(f'{who}: the solution has no regions')
    n_t = _n_theta(solution)
    if n_t > MAX_DIM:
        raise ValueError(f'{who}: n_theta = {n_t} > {MAX_DIM}')
    if not (numpy.isfinite(tol) and tol >= 0.0):
        raise ValueError(f'{who}: tol must be finite and >= 0')
    rows = output_rows(solution, outputs, who)
    ef, row_off, _ = solution._stacked()
    ef = numpy.asarray(ef, dtype=numpy.float64).reshape(-1, n_t + 1)
    nrm = numpy.linalg.norm(ef[:, 1:], axis=1)
    real = nrm > 0.0                                         # a row without a normal takes no part, as in reduce_rows
    counts = numpy.add.reduceat(real.astype(numpy.int64), row_off[:-1])
    counts[numpy.diff(row_off) == 0] = 0
    if counts.min() < 1:
        raise ValueError(f'{who}: region {int(numpy.argmin(counts))} has no row with a normal (the whole space, or nothing)')
    if counts.max() > MAX_ROWS:
        raise ValueError(f'{who}: region {int(numpy.argmax(counts))} has more than {MAX_ROWS} rows')
    unit = ef[real] / nrm[real, None]
    off = numpy.concatenate([[0], numpy.cumsum(counts)]).astype(numpy.int64)
    laws = _laws(solution, rows, n_t)                        # [R, K, n_t + 1] = [b | A]
    R, K = laws.shape[0], laws.shape[1]
    dirs = numpy.empty((R, K, 2, n_t))
    dirs[:, :, 0], dirs[:, :, 1] = laws[:, :, 1:], -laws[:, :, 1:]
    doff = (numpy.arange(R + 1) * (2 * K)).astype(numpy.int64)
    sv = support_of(off, unit, n_t, doff, dirs.reshape(-1, n_t), tol=tol, device=device, who=who)
    value, arg, st = sv.value.reshape(R, K, 2), sv.arg.reshape(R, K, 2, n_t), sv.dir_status.reshape(R, K, 2)
    b = laws[:, :, 0]
    return OutputRange(outputs=list(rows), lo=b - value[:, :, 1], hi=b + value[:, :, 0], arg_lo=arg[:, :, 1].copy(), arg_hi=arg[:, :, 0].copy(),
                       flag=numpy.any((st == UNBOUNDED) | (st == CAPPED), axis=2), thin=sv.poly_status == THIN, stats=dict(sv.stats))
