"""The exact largest difference between two explicit solutions (Solution.compare).

Two solutions A and B over the same parameter space, with regions R_i = {E_i theta <= f_i} and laws x = A_i theta + b_i restricted to the
same K output rows.  For a region i of A and a region j of B:

  X_ij     R_i n R_j, r_ij its Chebyshev radius.  r_ij <= tol: the pair does not meet (facet neighbours, disjoint regions).
  delta_k  (A_i[k] - A_j[k]).theta + (b_i[k] - b_j[k]) for output row k; lo_k = min, hi_k = max of delta_k over X_ij.
  gap_ij   max_k max(-lo_k, hi_k): the largest |x_A - x_B| on X_ij in any output row.  A maximum of an affine function over a polytope
           lies at a vertex of X_ij, where sampled points never fall; here it is the optimum of an LP.
  row_ij   the lowest k that attains the gap; witness_ij the theta where that LP ended.
  constant a row with A_i[k] == A_j[k] in every entry (compared as doubles, no threshold) needs no LP: lo = hi = b_i[k] - b_j[k], and a
           gap it gives has the Chebyshev centre of X_ij as its witness.  A self-comparison runs no law LP at all.
  flag     1: a bound, not a value.  An unbounded or capped radius run gives radius +inf (or the value reached), gap +inf, row -1; an
           unbounded or capped law LP gives lo = -inf or hi = +inf, hence gap +inf.

Stages: unit rows of both solutions in ONE region table (A's regions, then B's); feasible points and boxes (_lib.merge_regions);
candidate pairs by _pairs.candidate_pairs: boxes that overlap by more than tol in every coordinate (cross_box_pairs, a host sweep, or with
sweep='device' geometry.box_pairs); with screen='rows' the candidates that one row of either region separates from the other's box are dropped
(geometry.screen_pairs); per remaining candidate the radius LP and up to 2 K law LPs on the device (csrc/compare.hpp,
k_law_gap, one wavefront per pair).

Out of scope: gaps of value functions (a difference of quadratics is no LP), jumps across shared facets (radius 0), solutions flagged
overlapping (reduce them with remove_overlaps first).
"""
import time
from dataclasses import dataclass, field
from typing import Optional

import numpy

from ._pairs import (MAX_ROWS, candidate_pairs, check_pair_indices, check_polytopes, check_region_limits, check_rows_finite, check_scalars,
                     feasible_points, host_pairs)
from .region_merge import solution_rows

__all__ = ['LawGap', 'compare_solutions', 'law_gap_pairs', 'cross_box_pairs', 'output_rows', 'MAX_OUTPUTS']

MAX_OUTPUTS = 256     # LG_MAX_OUT of csrc/compare.hpp


def cross_box_pairs(box_a: numpy.ndarray, usable_a: numpy.ndarray, box_b: numpy.ndarray, usable_b: numpy.ndarray, tol: float):
    """(i, j), ascending by (i, j), with i a usable box of box_a [Ra, 2, n_t] (lower, upper) and j a usable box of box_b [Rb, 2, n_t] that
    overlap by more than tol in every coordinate.  One sweep along the first coordinate over both kinds of boxes together; infinite
    bounds are fine, and a NaN bound leaves its coordinate open."""
    return host_pairs('bound', box_a, usable_a, box_b, usable_b, tol)


def law_gap_pairs(row_off, ef_rows, laws, pair_a, pair_b, tol: float = 1e-8, xs=None, ranges: bool = False, device: int = 0) -> dict:
    """The pair stage on arrays: polytopes of unit rows ef_rows = [o | n] in CSR form by row_off (one table for both sides), laws
    [R, K, n_t + 1] = [b | A], and the pairs (pair_a[k], pair_b[k]) of polytopes.  ``xs`` [R, n_t]: where the radius run of a pair starts
    (polytope pair_a[k]'s row; any finite point); None: the feasible points of _lib.merge_regions.  ``ranges``: lo and hi of every row.

    Returns a dict: i, j (as given), radius, gap (NaN where the pair does not meet), row, witness [pairs, n_t], flag, ranges
    [pairs, K, 2] or None, and stats (pairs, meets, constant_rows, lps, pivots, wide, device_ms).  ValueError before anything reaches the
    device for shapes that do not fit, n_theta outside 1..16, K outside 1..256, a polytope without 1..256 rows, non-finite input, tol
    not finite or below 0 and pair indices out of range."""
    from . import _lib
    who = 'law_gap_pairs'
    off, ef, n_t, R = check_polytopes(who, row_off, ef_rows, max_rows=None)
    laws = numpy.asarray(laws, dtype=numpy.float64)
    if laws.ndim != 3 or laws.shape[0] != R or laws.shape[2] != n_t + 1:
        raise ValueError(f'{who}: laws must be [{R}, K, {n_t + 1}] = [b | A], not {list(laws.shape)}')
    if not 1 <= laws.shape[1] <= MAX_OUTPUTS:
        raise ValueError(f'{who}: the number of output rows K = {laws.shape[1]} is outside 1..{MAX_OUTPUTS}')
    check_scalars(who, n_t, tol)
    check_rows_finite(who, off, [ef, laws], word='laws')
    pa, pb = check_pair_indices(who, 'pair_a and pair_b', pair_a, pair_b, R)
    if xs is not None:
        xs = numpy.ascontiguousarray(xs, dtype=numpy.float64)
        if xs.shape != (R, n_t) or not numpy.all(numpy.isfinite(xs)):
            raise ValueError(f'{who}: xs must be a finite [{R}, {n_t}] array')
    stats = {'pairs': 0, 'meets': 0, 'constant_rows': 0, 'lps': 0, 'pivots': 0, 'wide': 0, 'pair_ms': 0.0, 'device_ms': 0.0}
    n = len(pa)
    if not n:
        return {'i': pa, 'j': pb, 'radius': numpy.zeros(0), 'gap': numpy.zeros(0), 'row': numpy.zeros(0, dtype=numpy.int32),
                'witness': numpy.zeros((0, n_t)), 'flag': numpy.zeros(0, dtype=numpy.int32),
                'ranges': numpy.zeros((0, laws.shape[1], 2)) if ranges else None, 'stats': stats}
    if xs is None:
        xs, _, _, s = _lib.merge_regions(off, ef, device)
        stats['device_ms'] += s['ms']
        xs = numpy.where(numpy.isfinite(xs), xs, 0.0)
    radius, gap, row, witness, rng, flag, s = _lib.law_gap_pairs(off, ef, laws, xs, pa, pb, tol, ranges=ranges, device=device)
    for k in _lib.LAW_GAP_KEYS:
        stats[k] = s[k]
    stats['pair_ms'] = s['ms']
    stats['device_ms'] += s['ms']
    return {'i': pa, 'j': pb, 'radius': radius, 'gap': gap, 'row': row, 'witness': witness, 'flag': flag, 'ranges': rng, 'stats': stats}


@dataclass
class LawGap:
    """What compare_solutions returns.  Per candidate pair k (ascending by (i, j)): region i[k] of A, region j[k] of B, radius[k] of their
    intersection, and where it exceeds tol gap[k], row[k] (the lowest output row, in the order of ``outputs``, that attains the gap) and
    witness[k] [n_t]; gap NaN and row -1 where the pair does not meet.  flag[k] = 1: a run was unbounded or capped and the gap (+inf) is
    a bound, not a value.  ranges [pairs, K, 2] = lo, hi of every row (None unless asked for).  covered_a, covered_b (None unless
    asked for): the share of every region's volume that lies in the meeting regions of the other side.
    stats: the kernel's counters (pairs, meets, constant_rows, lps, pivots, wide), device_ms, candidates, box_pairs (all pairs of usable
    regions, what the sweep spared the device), sweep_ms, wall_ms."""
    n_a: int
    n_b: int
    tol: float
    outputs: list
    i: numpy.ndarray
    j: numpy.ndarray
    radius: numpy.ndarray
    gap: numpy.ndarray
    row: numpy.ndarray
    witness: numpy.ndarray
    flag: numpy.ndarray
    usable_a: numpy.ndarray
    usable_b: numpy.ndarray
    ranges: Optional[numpy.ndarray] = None
    covered_a: Optional[numpy.ndarray] = None
    covered_b: Optional[numpy.ndarray] = None
    stats: dict = field(default_factory=dict)

    @property
    def meets(self) -> numpy.ndarray:
        """per pair: the intersection has a radius above tol (or its radius run was unbounded or capped)"""
        return ~numpy.isnan(self.gap)

    @property
    def argmax(self) -> int:
        """the first pair with the largest gap; -1 when nothing meets"""
        m = numpy.flatnonzero(self.meets)
        return int(m[numpy.argmax(self.gap[m])]) if len(m) else -1

    @property
    def max_gap(self) -> float:
        """the largest gap of any pair; 0.0 when nothing meets"""
        k = self.argmax
        return float(self.gap[k]) if k >= 0 else 0.0

    def worst(self, n: int = 10) -> numpy.ndarray:
        """the indices of the n meeting pairs with the largest gaps, largest first, ties in pair order"""
        m = numpy.flatnonzero(self.meets)
        return m[numpy.argsort(-self.gap[m], kind='stable')][:max(int(n), 0)]

    def _gap_of(self, idx: numpy.ndarray, n: int) -> numpy.ndarray:
        out = numpy.full(n, -numpy.inf)
        m = self.meets
        numpy.maximum.at(out, idx[m], self.gap[m])
        out[numpy.isneginf(out)] = numpy.nan
        return out

    @property
    def gap_of_a(self) -> numpy.ndarray:
        """[n_a] the largest gap of every region of A over its partners; NaN for a region that meets none"""
        return self._gap_of(self.i, self.n_a)

    @property
    def gap_of_b(self) -> numpy.ndarray:
        return self._gap_of(self.j, self.n_b)

    def _unmatched(self, idx: numpy.ndarray, usable: numpy.ndarray) -> numpy.ndarray:
        met = numpy.zeros(len(usable), dtype=bool)
        met[idx[self.meets]] = True
        return numpy.flatnonzero(usable & ~met)

    @property
    def unmatched_a(self) -> numpy.ndarray:
        """the usable regions of A that meet no region of B above tol, ascending"""
        return self._unmatched(self.i, self.usable_a)

    @property
    def unmatched_b(self) -> numpy.ndarray:
        return self._unmatched(self.j, self.usable_b)

    @property
    def wide(self) -> int:
        """the number of flagged pairs"""
        return int(numpy.count_nonzero(self.flag))

    def equal(self, atol: float = 0.0) -> bool:
        """max_gap <= atol, no flagged pair, and no region of either side without a partner"""
        return bool(self.max_gap <= atol) and self.wide == 0 and not len(self.unmatched_a) and not len(self.unmatched_b)


def _n_theta(solution) -> int:
    return solution.theta_dim() if solution.program is not None else numpy.asarray(solution.critical_regions[0].E).shape[1]


def output_rows(solution, outputs, who: str = 'compare') -> list:
    """Where the rows ``outputs`` of the program's x stand in the laws of this solution's regions: the rows themselves for a solution
    that keeps the full law, their places in merge_info['outputs'] for a merged one.  None: every row the regions keep.  ValueError for
    an empty list, a row out of range and a row the merged solution did not keep."""
    n_t = _n_theta(solution)
    n_rows = numpy.asarray(solution.critical_regions[0].A).reshape(-1, n_t).shape[0]
    if outputs is None:
        return list(range(n_rows))
    outputs = [int(o) for o in outputs]
    if not outputs:
        raise ValueError(f'{who}: outputs must be a non-empty list of row indices of x')
    if solution.merge_info is not None:
        kept = [int(o) for o in solution.merge_info['outputs']]
        for o in outputs:
            if o not in kept:
                raise ValueError(f'{who}: the merged solution kept the rows {kept} of x, not row {o}')
        return [kept.index(o) for o in outputs]
    for o in outputs:
        if not 0 <= o < n_rows:
            raise ValueError(f'{who}: outputs must be row indices of x in 0..{n_rows - 1}, got {o}')
    return outputs


def _laws(solution, rows, n_t: int) -> numpy.ndarray:
    """[R, K, n_t + 1] = [b | A] of the regions, restricted to the law rows ``rows``"""
    out = numpy.empty((len(solution.critical_regions), len(rows), n_t + 1))
    for k, r in enumerate(solution.critical_regions):
        out[k, :, 0] = numpy.asarray(r.b, dtype=numpy.float64).reshape(-1)[rows]
        out[k, :, 1:] = numpy.asarray(r.A, dtype=numpy.float64).reshape(-1, n_t)[rows]
    return out


def check_sources(a, b, outputs, tol: float):
    """(n_theta, law rows of a, law rows of b) of two solutions compare accepts; ValueError otherwise, before anything reaches the device."""
    who = 'compare'
    for name, s in (('this', a), ('the other', b)):
        if not s.critical_regions:
            raise ValueError(f'{who}: {name} solution has no regions')
        if s.is_overlapping:
            raise ValueError(f'{who}: {name} solution is flagged overlapping: a point may lie in several regions, and which law acts there '
                             f'is chosen by objective; reduce it with remove_overlaps() first')
    n_t, n_tb = _n_theta(a), _n_theta(b)
    if n_t != n_tb:
        raise ValueError(f'{who}: the solutions have different n_theta ({n_t} and {n_tb})')
    check_region_limits(who, (), n_t)
    if not (numpy.isfinite(tol) and tol >= 0.0):
        raise ValueError(f'{who}: tol must be finite and >= 0')
    check_region_limits(who, a.critical_regions, n_t, 'of this solution')
    check_region_limits(who, b.critical_regions, n_t, 'of the other solution')
    rows_a, rows_b = output_rows(a, outputs, who), output_rows(b, outputs, who)
    if len(rows_a) != len(rows_b):
        raise ValueError(f'{who}: the solutions keep {len(rows_a)} and {len(rows_b)} rows of x: name the rows to compare with outputs')
    if len(rows_a) > MAX_OUTPUTS:
        raise ValueError(f'{who}: more than {MAX_OUTPUTS} output rows')
    return n_t, rows_a, rows_b


def _coverage(off, rows, n_t, n_a, res, tol, device):
    """(covered_a, covered_b): per region the summed volume of its unflagged meeting intersections over its own volume"""
    from .geometry.polytope import Polytope
    from .geometry.reduce import reduce_rows_of
    from .geometry.volume import polytope_volumes
    who = 'compare (coverage)'
    R = len(off) - 1
    take = numpy.flatnonzero((res['radius'] > tol) & (res['flag'] == 0))
    gi, gj = res['i'][take], res['j'][take] + n_a
    polys = [Polytope(rows[off[r]:off[r + 1], 1:].copy(), rows[off[r]:off[r + 1], :1].copy()) for r in range(R)]
    if len(take):
        parts = [numpy.vstack([rows[off[p]:off[p + 1]], rows[off[q]:off[q + 1]]]) for p, q in zip(gi.tolist(), gj.tolist())]
        poff = numpy.concatenate([[0], numpy.cumsum([len(p) for p in parts])]).astype(numpy.int64)
        red = reduce_rows_of(poff, numpy.vstack(parts), n_t, tol=tol, start=res['witness'][take], device=device, who=who)
        if int(numpy.diff(red.row_off).max()) > MAX_ROWS:
            raise ValueError(f'{who}: an intersection keeps more than {MAX_ROWS} rows, the limit of polytope_volumes')
        polys = polys + red.polytopes()
    vol = polytope_volumes(polys, device=device).volume
    shared = numpy.zeros(R)
    numpy.add.at(shared, gi, vol[R:])
    numpy.add.at(shared, gj, vol[R:])
    with numpy.errstate(invalid='ignore', divide='ignore'):
        covered = shared / vol[:R]
    return covered[:n_a], covered[n_a:]


def compare_solutions(a, b, outputs=None, tol: float = 1e-8, ranges: bool = False, coverage: bool = False, device: int = 0,
                      sweep: str = 'host', screen: str = 'none') -> LawGap:
    """Solution.compare (the module docstring): a LawGap between the laws of ``a`` and ``b`` on the rows ``outputs`` of the program's x
    (None: all rows, which then must be equal in number on both sides).  For a merged solution, whose regions keep only
    merge_info['outputs'], the rows are mapped onto the ones it kept.  ``coverage``: covered_a[i] = sum_j vol(X_ij) / vol(R_i) and
    covered_b likewise, by geometry.reduce_rows_of on the stacked rows of the meeting pairs and geometry.polytope_volumes; exact when the
    other side does not overlap itself, and within their limits (ValueError naming the one that was hit).  Neither solution is modified.
    ``sweep`` = 'device': the candidates come from geometry.box_pairs instead of cross_box_pairs, the same list, so every result is the
    same bit for bit.  ``screen`` = 'rows': candidates that a single row separates from the partner's box never reach the LPs; the
    per-pair arrays then hold the kept candidates only (every meeting pair is among them), and stats gains box_candidates, screened
    and screen_ms.  ValueError for any other value."""
    from .geometry.box_pairs import sweep_options
    sweep_options('compare', sweep, screen)
    t0 = time.perf_counter()
    n_t, rows_a, rows_b = check_sources(a, b, outputs, tol)
    off_a, ef_a, void_a = solution_rows(a.critical_regions, n_t, 'compare')
    off_b, ef_b, void_b = solution_rows(b.critical_regions, n_t, 'compare')
    n_a, n_b = len(off_a) - 1, len(off_b) - 1
    off = numpy.concatenate([off_a, off_b[1:] + off_a[-1]]).astype(numpy.int64)
    ef = numpy.vstack([ef_a, ef_b])
    laws = numpy.concatenate([_laws(a, rows_a, n_t), _laws(b, rows_b, n_t)])
    if not numpy.all(numpy.isfinite(laws)):
        raise ValueError('compare: the laws must be finite')
    xs, box, usable, s = feasible_points(off, ef, list(void_a) + [n_a + i for i in void_b], device)
    pa, pb, swept = candidate_pairs('compare', 'bound', box[:n_a], usable[:n_a], box[n_a:], usable[n_a:], tol, off, ef, lambda: (box, box), 'both',
                                    sweep, screen, device, shift=n_a)
    res = law_gap_pairs(off, ef, laws, pa, pb + n_a, tol=tol, xs=xs, ranges=ranges, device=device)
    res['i'], res['j'] = pa, pb
    stats = dict(res['stats'])
    stats['device_ms'] += s['ms']
    stats.update(candidates=len(pa), box_pairs=int(usable[:n_a].sum()) * int(usable[n_a:].sum()), **swept)
    covered_a = covered_b = None
    if coverage:
        covered_a, covered_b = _coverage(off, ef, n_t, n_a, res, tol, device)
    stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
    shown = list(range(len(rows_a))) if outputs is None else [int(o) for o in outputs]
    return LawGap(n_a=n_a, n_b=n_b, tol=float(tol), outputs=shown, i=pa, j=pb, radius=res['radius'], gap=res['gap'], row=res['row'],
                  witness=res['witness'], flag=res['flag'], usable_a=usable[:n_a].copy(), usable_b=usable[n_a:].copy(), ranges=res['ranges'],
                  covered_a=covered_a, covered_b=covered_b, stats=stats)
