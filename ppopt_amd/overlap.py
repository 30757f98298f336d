"""Partitioning an overlapping solution by lowest objective (Solution.remove_overlaps).

Every mpLP solution, and every mixed-integer one with more than one parameter, is overlapping: a parameter point may lie in several
regions R_i = {E_i theta <= f_i} and the answer there is the one with the lowest value J_i(theta).  When all value functions share
one quadratic part, J_i - J_j is affine and "i is cheaper than j" is a half-space, so the comparison procedure of the mpMILP
literature needs LPs only.  Region i owns theta in R_i iff for every other j with theta in R_j: J_i < J_j, or J_i = J_j and i > j (the
tie rule of Solution.get_region).  The procedure is deterministic:

  1. unit rows [o | n] of every region (region_merge.unit_rows); feasible points and bounding boxes by _lib.merge_regions;
  2. D = J_i - J_j = g.theta + h.  The pair is value-equal when |g| <= value_tol (1 + max |qv|) and |h| <= value_tol (1 + max |rv|);
     with |g| that small and |h| not, the cheaper region is cheaper everywhere (d_min = d_max = +-inf by the sign of h, no LP);
     otherwise the cut row of the pair is the unit row of {J_j <= J_i}, [h / |g| | -g / |g|], and d(theta) = (J_i - J_j) / |g| the depth
     behind it;
  3. candidate pairs i < j by _pairs.candidate_pairs: boxes overlapping by more than tol in every coordinate (box_pairs, a host sweep, or
     with sweep='device' geometry.box_pairs; screen='rows' drops the candidates that a row of one region separates from the other's box,
     DESIGN §3.27).  On the device (csrc/overlap.hpp,
     k_overlap_pairs): r = the Chebyshev radius of R_i n R_j, and d_min, d_max over it.  Verdicts, first match:
       a radius run unbounded or capped  EQUAL when value-equal, else CROSSING      r <= tol          DISJOINT
       value-equal                       EQUAL    (i is cut by R_j)                  d_max <= tol      I_WINS  (j is cut by R_i)
       d_min >= -tol                     J_WINS   (i is cut by R_j)                  a d run unbounded or capped, or neither: CROSSING
     CROSSING: i is cut by R_j and the cut row, j by R_i and the reversed cut row;
  4. region i's cutters in ascending j; pieces start as [R_i]; in round r every live piece of a region with more than r cutters meets
     its r-th cutter C (rows c_1 .. c_p: the region's, then the cut row), one launch per round (k_overlap_split): where
     radius(P n C) <= tol the piece stays; otherwise the children P n {earlier cutting rows} n {n_k.theta >= o_k} for every row k
     that cuts (the child's radius exceeds tol) replace it in row order, with rows: P's, the earlier cutting rows, the reversed row.

The pieces of one source are convex, closed, and share boundaries only; they are not merged back.  They keep redundant rows unless
``reduce_rows`` is set, which removes them round by round (geometry/reduce.py; off by default).
"""
import time
from dataclasses import dataclass
from typing import List, Optional

import numpy

from .critical_region import CriticalRegion
from ._pairs import MAX_ROWS, candidate_pairs, check_polytopes, check_region_limits, check_scalars, feasible_points, host_pairs
from .region_merge import mask_rows, solution_rows

__all__ = ['ReducedRegion', 'OverlapPartition', 'remove_overlaps', 'partition_by_value', 'difference_rounds', 'build_reduced_solution', 'VERDICTS']

VERDICTS = ('DISJOINT', 'EQUAL', 'I_WINS', 'J_WINS', 'CROSSING')
DISJOINT, EQUAL, I_WINS, J_WINS, CROSSING = range(5)


@dataclass(eq=False)
class ReducedRegion(CriticalRegion):
    """A piece of region ``source`` of the solution remove_overlaps was given: the source's laws, active set and binaries on the part
    {E theta <= f} of the source region where its value is the lowest."""
    source: int = -1


@dataclass
class OverlapPartition:
    """What partition_by_value returns.  pieces[k]: unit rows [o | n] of piece k, or None for a source that lost nothing (its own rows
    stand); sources[k]: its source; pairs: (i, j, verdict, radius, d_min, d_max) arrays of the candidate pairs."""
    pieces: List[Optional[numpy.ndarray]]
    sources: numpy.ndarray
    vanished: List[int]
    pairs: dict
    verdict_counts: dict
    stats: dict


def box_pairs(box: numpy.ndarray, usable: numpy.ndarray, tol: float):
    """(i, j) with i < j, ascending, of the usable regions whose boxes [R, 2, n_t] overlap by more than tol in every coordinate: a sweep
    along the first coordinate."""
    return host_pairs('mask', box, usable, None, None, tol)


def classify_pairs(radius, d_min, d_max, flag, equal, tol: float) -> numpy.ndarray:
    """The host verdicts of step 3 from what k_overlap_pairs wrote (d_min, d_max NaN where it ran no d LP and the host filled none)."""
    n = len(radius)
    v = numpy.full(n, CROSSING, dtype=numpy.int32)
    with numpy.errstate(invalid='ignore'):
        radius_open = (flag != 0) & numpy.isnan(d_min)            # the radius run itself was unbounded or capped
        done = numpy.zeros(n, dtype=bool)
        for cond, verdict in ((radius_open & equal, EQUAL), (radius_open & ~equal, CROSSING), (radius <= tol, DISJOINT), (equal, EQUAL),
                              ((flag == 0) & (d_max <= tol), I_WINS), ((flag == 0) & (d_min >= -tol), J_WINS)):
            take = cond & ~done
            v[take] = verdict
            done |= take
    return v


def difference_rounds(who, off, ef, xs, usable, cutters, launch, cutting_rows, max_pieces: int, stats: dict, items_key: str, reduce=None):
    """The rounds of a region difference (step 4 of the module docstring; exit_sets.py runs the same rounds against pulled-back
    cutters).  cutters[i]: the entries (cutter region j, extra row or None) that polytope i meets, one per round, in order.
    ``launch(piece_off, piece_rows, item_source, item_entries, item_start)`` runs the items of a round, item k being piece k, and returns
    (flag, mask, stats) of the library's split call; ``cutting_rows(source, entry, mask, flag)`` gives the ordered rows that cut an item
    whose piece meets its cutter.  Returns (live, round_ms): per source its pieces in order as (rows, or None for the source's own rows,
    wide: a run on the way to the piece was unbounded or capped), and the device ms of every round.  rounds, ``items_key``, lps, pivots,
    wide, device_ms and max_item_rows are accumulated into ``stats``; ValueError in the name of ``who`` past MAX_ROWS or max_pieces.
    ``reduce(piece_off, piece_rows, start)``, when given, answers like _lib.reduce_rows (kept per row, status, wide, point, stats): the
    children made in a round lose their redundant rows in one call per round, started from the source's point of xs, before the MAX_ROWS
    check, which then applies to the reduced pieces; a child found thin is dropped, a wide one flags its piece, and ``stats`` gains
    reduce_lps, reduce_ms and rows_removed (geometry/reduce.py)."""
    from . import _lib
    R, counts = len(off) - 1, numpy.diff(off)
    if reduce is not None:
        for k in ('reduce_lps', 'reduce_ms', 'rows_removed'):
            stats.setdefault(k, 0.0 if k == 'reduce_ms' else 0)
    live = [[(None, False)] if usable[i] else [] for i in range(R)]
    round_ms = []
    for rnd in range(max((len(c) for c in cutters), default=0)):
        active = [i for i in range(R) if len(cutters[i]) > rnd and live[i]]
        if not active:
            continue
        p_rows, item_source, entries = [], [], []
        for i in active:
            for pc, _ in live[i]:
                p_rows.append(ef[off[i]:off[i + 1]] if pc is None else pc)
                item_source.append(i)
                entries.append(cutters[i][rnd])
        p_counts = [len(rows) for rows in p_rows]
        poff = numpy.concatenate([[0], numpy.cumsum(p_counts)]).astype(numpy.int64)
        fl, mask, s = launch(poff, numpy.vstack(p_rows), item_source, entries, numpy.asarray([xs[i] for i in item_source]))
        stats['rounds'] += 1
        stats[items_key] += len(p_rows)
        stats['max_item_rows'] = max(stats['max_item_rows'], max(m + int(counts[j]) + (c is not None) for m, (j, c) in zip(p_counts, entries)))
        for k in ('lps', 'pivots', 'wide'):
            stats[k] += s[k]
        stats['device_ms'] += s['ms']
        round_ms.append(s['ms'])
        q = 0
        fresh = []     # (source, place in live[source]) of the children of this round, for ``reduce``
        for i in active:
            nxt = []
            for pc, wide in live[i]:
                if not fl[q] & _lib.OVERLAP_MEETS:
                    nxt.append((pc, wide))
                else:
                    cutting = cutting_rows(i, entries[q], mask[q], int(fl[q]))
                    w = wide or bool(fl[q] & _lib.OVERLAP_WIDE)
                    for k, row in enumerate(cutting):
                        if reduce is not None:
                            fresh.append((i, len(nxt)))
                        nxt.append((numpy.vstack([p_rows[q]] + cutting[:k] + [-row]), w))
                q += 1
            live[i] = nxt
        if fresh:
            c_rows = [live[i][k][0] for i, k in fresh]
            if max(len(rows) for rows in c_rows) > _lib.REDUCE_MAX_ROWS:
                raise ValueError(f'{who}: a piece has more than {MAX_ROWS} rows after round {rnd + 1}')
            coff = numpy.concatenate([[0], numpy.cumsum([len(rows) for rows in c_rows])]).astype(numpy.int64)
            kept, c_status, c_wide, _, s = reduce(coff, numpy.vstack(c_rows), numpy.asarray([xs[i] for i, _ in fresh]))
            stats['reduce_lps'] += s['lps']
            stats['reduce_ms'] += s['ms']
            stats['rows_removed'] += int(numpy.sum(~kept))
            gone = set()
            for n, (i, k) in enumerate(fresh):
                if c_status[n] == _lib.REDUCE_THIN:
                    gone.add((i, k))
                else:
                    live[i][k] = (c_rows[n][kept[coff[n]:coff[n + 1]]], live[i][k][1] or bool(c_wide[n]))
            if gone:
                for i in active:
                    live[i] = [p for k, p in enumerate(live[i]) if (i, k) not in gone]
        if any(pc is not None and len(pc) > MAX_ROWS for i in active for pc, _ in live[i]):
            raise ValueError(f'{who}: a piece has more than {MAX_ROWS} rows after round {rnd + 1}')
        if sum(len(p) for p in live) > max_pieces:
            raise ValueError(f'{who}: more than max_pieces = {max_pieces} pieces after round {rnd + 1}')
    return live, round_ms


def partition_by_value(row_off, ef_rows, g, h, n_t: int, tol: float = 1e-8, value_tol: float = 1e-9, max_pieces: int = 1 << 20,
                       device: int = 0, void=(), reduce_rows: bool = False, sweep: str = 'host', screen: str = 'none') -> OverlapPartition:
    """The partition of the polytopes {n.theta <= o} (unit rows ef_rows = [o | n] in CSR form by row_off) by the lowest affine value
    g_i.theta + h_i: an OverlapPartition.  Steps 2 to 4 of the module docstring; every LP runs on the device.  ``void``: polytopes
    known to be empty (they vanish and cut nothing), like the ones the device finds empty.  ``reduce_rows``: the children of every
    round lose their redundant rows (difference_rounds, ``reduce``).  ``sweep`` = 'device': the candidates of step 3 come from
    geometry.box_pairs, the same list as box_pairs gives; ``screen`` = 'rows': the candidates that a single row separates from the partner's
    box never reach the pair stage (they could only be DISJOINT), ``pairs`` holds the kept ones and stats gains box_candidates, screened,
    screen_ms.  With either, stats also holds sweep_ms, the wall time of the sweep."""
    from . import _lib
    from .geometry.box_pairs import sweep_options
    sweep_options('partition_by_value', sweep, screen)
    t0 = time.perf_counter()
    check_scalars('partition_by_value', n_t)
    if not (numpy.isfinite(tol) and tol >= 0.0 and numpy.isfinite(value_tol) and value_tol >= 0.0):
        raise ValueError('partition_by_value: tol and value_tol must be finite and >= 0')
    g = numpy.ascontiguousarray(g, dtype=numpy.float64).reshape(-1, n_t)
    h = numpy.ascontiguousarray(h, dtype=numpy.float64).reshape(-1)
    off, ef, _, R = check_polytopes('partition_by_value', row_off, ef_rows, n_t, extra=[('g [R, n_t]', g, (n_t,)), ('h [R]', h, ())], word='values')
    stats = {'regions_before': R, 'candidate_pairs': 0, 'rounds': 0, 'work_items': 0, 'max_item_rows': 0, 'lps': 0, 'pivots': 0, 'wide': 0, 'device_ms': 0.0}
    xs, box, usable, s = feasible_points(off, ef, void, device)
    stats['lps'] += s['lps']
    stats['pivots'] += s['pivots']
    stats['device_ms'] += s['ms']
    # 2. values
    pa, pb, swept = candidate_pairs('partition_by_value', 'mask', box, usable, None, None, tol, off, ef, lambda: (box, box), 'both', sweep, screen, device)
    if (sweep, screen) == ('host', 'none'):
        del swept['sweep_ms']      # reported with the device sweep or the screen only
    stats.update(swept)
    n_pairs = len(pa)
    stats['candidate_pairs'] = n_pairs
    g_thr = value_tol * (1.0 + float(numpy.max(numpy.linalg.norm(g, axis=1))))
    h_thr = value_tol * (1.0 + float(numpy.max(numpy.abs(h))))
    dg, dh = g[pa] - g[pb], h[pa] - h[pb]
    gn = numpy.linalg.norm(dg, axis=1)
    flat = gn <= g_thr
    equal = flat & (numpy.abs(dh) <= h_thr)
    has_cut = ~flat
    safe = numpy.where(has_cut, gn, 1.0)
    cut = numpy.hstack([(dh / safe).reshape(-1, 1), -dg / safe[:, None]])
    cut[~has_cut] = 0.0
    # 3. the pair stage
    if n_pairs:
        radius, d_min, d_max, flag, s = _lib.overlap_pairs(off, ef, xs, pa, pb, has_cut.astype(numpy.int32), cut, tol, device)
        for k in ('lps', 'pivots'):
            stats[k] += s[k]
        stats['wide'] += s['capped']
        stats['device_ms'] += s['ms']
    else:
        radius = d_min = d_max = numpy.zeros(0)
        flag = numpy.zeros(0, dtype=numpy.int32)
    const = flat & ~equal & (flag == 0)      # a constant difference: the sign of h decides everywhere
    d_min, d_max = d_min.copy(), d_max.copy()
    d_min[const] = d_max[const] = numpy.where(dh[const] > 0.0, numpy.inf, -numpy.inf)
    radius_open = (flag != 0) & numpy.isnan(d_min)
    verdict = classify_pairs(radius, d_min, d_max, flag, equal, tol)
    # a constant difference behind an open radius run has no cut row to cross at: the cheaper region cuts the other
    fix = radius_open & flat & ~equal
    verdict[fix] = numpy.where(dh[fix] > 0.0, J_WINS, I_WINS)
    cutters = [[] for _ in range(R)]          # (cutter region, cut row or None), ascending by cutter
    for k in numpy.flatnonzero(verdict != DISJOINT).tolist():
        i, j, v = int(pa[k]), int(pb[k]), int(verdict[k])
        if v in (EQUAL, J_WINS):
            cutters[i].append((j, None))
        elif v == I_WINS:
            cutters[j].append((i, None))
        else:
            cutters[i].append((j, cut[k]))
            cutters[j].append((i, -cut[k]))
    for c in cutters:
        c.sort(key=lambda jc: jc[0])
    # 4. the difference stage
    def launch(poff, prows, item_source, entries, start):
        zero = numpy.zeros(n_t + 1)
        return _lib.overlap_split(off, ef, poff, prows, numpy.arange(len(entries)), [j for j, _ in entries], [0 if c is None else 1 for _, c in entries],
                                  numpy.asarray([zero if c is None else c for _, c in entries]), start, tol, device)

    def cutting_rows(i, entry, mask, flag):
        j, c = entry
        cj = ef[off[j]:off[j + 1]]
        return [cj[r] for r in mask_rows(mask, len(cj)).tolist()] + ([c] if flag & _lib.OVERLAP_CUT_ROW else [])

    reduce = (lambda poff, prows, start: _lib.reduce_rows(poff, prows, start, tol, device)) if reduce_rows else None
    live, _ = difference_rounds('remove_overlaps', off, ef, xs, usable, cutters, launch, cutting_rows, max_pieces, stats, 'work_items', reduce=reduce)
    live = [[pc for pc, _ in p] for p in live]
    pieces = [pc for i in range(R) for pc in live[i]]
    sources = numpy.asarray([i for i in range(R) for _ in live[i]], dtype=numpy.int64)
    counts_v = {name: int(numpy.sum(verdict == k)) for k, name in enumerate(VERDICTS)}
    stats['regions_after'] = len(pieces)
    stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
    return OverlapPartition(pieces=pieces, sources=sources, vanished=[i for i in range(R) if not live[i]],
                            pairs={'i': pa, 'j': pb, 'verdict': verdict, 'radius': radius, 'd_min': d_min, 'd_max': d_max},
                            verdict_counts=counts_v, stats=stats)


def build_reduced_solution(source, sources, rows, verdict_counts: Optional[dict] = None, vanished=None, stats: Optional[dict] = None):
    """The reduced Solution from ``sources`` (non-decreasing source index per piece) and ``rows`` (per piece [m, n_t + 1] unit rows
    [o | n], or None for a source that lost nothing, whose E, f are copied unchanged).  Host only: no device is touched."""
    from .solution import Solution
    regs = source.critical_regions
    n_t = source.theta_dim() if source.program is not None else numpy.asarray(regs[0].E).shape[1]
    sources = numpy.asarray(sources, dtype=numpy.int64).reshape(-1)
    if len(sources) != len(rows) or numpy.any(sources < 0) or numpy.any(sources >= len(regs)) or numpy.any(numpy.diff(sources) < 0):
        raise ValueError('build_reduced_solution: sources must be non-decreasing indices into the source regions, one per piece')
    copy = lambda a: None if a is None else numpy.array(a, copy=True)
    out = []
    for i, rk in zip(sources.tolist(), rows):
        src = regs[i]
        if rk is None:
            E, f = numpy.array(src.E, dtype=numpy.float64, copy=True), numpy.array(src.f, dtype=numpy.float64, copy=True)
        else:
            rk = numpy.asarray(rk, dtype=numpy.float64).reshape(-1, n_t + 1)
            E, f = rk[:, 1:].copy(), rk[:, :1].copy()
        out.append(ReducedRegion(copy(src.A), copy(src.b), copy(src.C), copy(src.d), E, f, list(src.active_set), list(src.omega_set),
                                 list(src.lambda_set), [list(v) for v in src.regular_set], copy(src.y_fixation), copy(src.y_indices),
                                 copy(src.x_indices), source=int(i)))
    sol = Solution(source.program, out, is_overlapping=False, point_location_tolerance=source.point_location_tolerance)
    sol.is_complete = source.is_complete
    present = set(sources.tolist())
    sol.overlap_info = {'source': source, 'sources': sources.copy(), 'verdict_counts': dict(verdict_counts or {}),
                        'vanished': sorted(int(i) for i in vanished) if vanished is not None else
                        [i for i in range(len(regs)) if i not in present], 'stats': dict(stats or {})}
    return sol


def check_source(source, tol: float, value_tol: float, max_pieces: int):
    """(n_theta, qv, rv) of a solution remove_overlaps accepts; ValueError otherwise, before anything reaches the device."""
    if not source.critical_regions:
        raise ValueError('remove_overlaps: the solution has no regions')
    if source.merge_info is not None:
        raise ValueError('remove_overlaps: a merged solution keeps no full law to compare values with: reduce the source '
                         '(merge_info["source"]) instead')
    n_t = source.theta_dim() if source.program is not None else numpy.asarray(source.critical_regions[0].E).shape[1]
    check_region_limits('remove_overlaps', source.critical_regions, n_t)
    if not (numpy.isfinite(tol) and tol >= 0.0 and numpy.isfinite(value_tol) and value_tol >= 0.0):
        raise ValueError('remove_overlaps: tol and value_tol must be finite and >= 0')
    if int(max_pieces) < 1:
        raise ValueError('remove_overlaps: max_pieces must be >= 1')
    Qv, qv, rv = source.value_function()
    if numpy.max(numpy.abs(Qv - Qv[0])) > value_tol * (1.0 + numpy.max(numpy.abs(Qv))):
        raise ValueError('remove_overlaps: the value functions do not share one quadratic part; the comparison of quadratic value '
                         'functions is not convex and is out of scope (mpLP and mpMILP solutions without bilinear terms qualify)')
    return n_t, qv, rv


def remove_overlaps(source, tol: float = 1e-8, value_tol: float = 1e-9, max_pieces: int = 1 << 20, device: int = 0, reduce_rows: bool = False,
                    sweep: str = 'host', screen: str = 'none'):
    """Solution.remove_overlaps (the module docstring).  Returns a new Solution of ReducedRegion; the source is not modified.
    ``reduce_rows``: the pieces lose their redundant rows round by round (partition_by_value).  ``sweep``, ``screen``: where the candidate
    pairs come from and whether rows screen them (partition_by_value); the reduced solution is the same either way."""
    from .geometry.box_pairs import sweep_options
    sweep_options('remove_overlaps', sweep, screen)
    t0 = time.perf_counter()
    n_t, qv, rv = check_source(source, tol, value_tol, max_pieces)
    off, rows, void = solution_rows(source.critical_regions, n_t, 'remove_overlaps')
    part = partition_by_value(off, rows, qv, rv, n_t, tol=tol, value_tol=value_tol, max_pieces=max_pieces, device=device,
                              void=void, reduce_rows=reduce_rows, sweep=sweep, screen=screen)
    part.stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
    return build_reduced_solution(source, part.sources, part.pieces, part.verdict_counts, part.vanished, part.stats)
