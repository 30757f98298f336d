"""Exit sets of an explicit controller in closed loop (Solution.exit_sets): where each region's next state leaves the
solution.

On region R_i = {n.theta <= o} (unit rows [o | n]) the loop is affine, theta+ = Phi_i theta + phi_i (invariance.closed_loop_maps).

  pulled-back cutter  C_ij = {theta : Phi_i theta + phi_i in R_j}.  Its rows are the pulled-back rows of the transition graph
                      (transition.py): a row [o | n] of R_j becomes a.theta <= beta with a = Phi_i^T n, beta = o - n.phi_i, s = |a|; with
                      s > 1e-12 max(1, max |Phi_i|) it is the unit row [beta / s | a / s], otherwise it is constant: beta < -tol empties
                      C_ij (the piece stays, no LP), any other constant row is dropped and never cuts.
  exit set            X_i = R_i \\ U_j C_ij, reported as convex pieces of Chebyshev radius > tol.  Thinner parts are not reported, so every
                      statement holds for almost every state.  A radius run that is unbounded or stopped at the pivot cap counts as
                      "cuts": the child is kept and flagged wide; the pieces then over-approximate X_i and never lose a state that exits.

The procedure is deterministic, the difference of overlap.py step 4 against pulled-back cutters:

  1. region i's cutters are its successors j in the transition graph of the same (A, B, inputs, c, tol), ascending; every edge status
     counts.  A region that is no successor cannot hold an image of radius above tol, so it cuts nothing.
  2. pieces start as [R_i]; in round r every live piece P of a region with more than r successors meets C_ij of its r-th successor, one
     launch per round (csrc/exit_sets.hpp, k_exit_split): where radius(P n C) <= tol the piece stays; otherwise the children
     P n {earlier cutting rows} n {reversed row k} for every cutter row k that cuts (the child's radius exceeds tol) replace it in row
     order, with rows: P's, the earlier cutting rows, the reversed row; P n C is dropped.
  3. pieces the device finds empty (only a wide one can be) are dropped.

The pieces of one region are convex, closed, and share boundaries only; they are not merged back.  They keep redundant rows unless
``reduce_rows`` is set, which removes them round by round, or ExitSets.reduced() is called on the result (geometry/reduce.py, DESIGN
§3.22; off by default).
"""
import time
from dataclasses import dataclass, field
from typing import List, Optional

import numpy

from .overlap import difference_rounds
from ._pairs import check_polytopes, check_scalars, feasible_points, map_entries
from .region_merge import mask_rows, solution_rows

__all__ = ['ExitSets', 'ExitVolumes', 'exit_sets', 'exit_pieces', 'pulled_back_rows', 'ROW_EPS']

ROW_EPS = 1e-12        # TS_ROW_EPS of csrc/transition.hpp


def pulled_back_rows(rows_j, Phi_i, phi_i):
    """[m_j, n_t + 1]: the rows [o | n] of a target region pulled back through theta+ = Phi_i theta + phi_i and scaled to unit normals;
    a constant row (see the module docstring) is NaN."""
    a = rows_j[:, 1:] @ Phi_i
    beta = rows_j[:, 0] - rows_j[:, 1:] @ phi_i
    s = numpy.sqrt(numpy.sum(a * a, axis=1))
    keep = s > ROW_EPS * max(1.0, float(numpy.max(numpy.abs(Phi_i))))
    out = numpy.full((len(rows_j), rows_j.shape[1]), numpy.nan)
    out[keep] = numpy.column_stack([beta[keep] / s[keep], a[keep] / s[keep, None]])
    return out


@dataclass
class ExitVolumes:
    """piece [pieces]: the volume of every piece; exit [n_regions]: their sum per region (0 without a piece); region [n_regions]: the
    region's own volume; share = exit / region; total_share: the summed exit volume over the summed region volume.  NaN where the volume
    pass gives no answer (geometry.volume: OVERFLOW, TOO_LARGE, INCONSISTENT, or an unbounded region)."""
    piece: numpy.ndarray
    exit: numpy.ndarray
    region: numpy.ndarray
    share: numpy.ndarray
    total_share: float
    piece_status: numpy.ndarray
    region_status: numpy.ndarray


@dataclass
class ExitSets:
    """The exit pieces in CSR form: piece k has the unit rows [o | n] piece_rows[piece_off[k]:piece_off[k + 1]] and lies in region
    source[k] (non-decreasing); wide[k]: a radius run on the way to it was unbounded or capped, the piece may hold states that stay.
    whole[i]: region i has a piece that lost nothing (its own rows).  stats: rounds, items, lps, pivots, wide, pieces, device_ms,
    round_ms (device ms per round) and wall_ms.  region_off, region_rows: the regions the pieces were cut from."""
    n_regions: int
    piece_off: numpy.ndarray
    piece_rows: numpy.ndarray
    source: numpy.ndarray
    wide: numpy.ndarray
    whole: numpy.ndarray
    stats: dict = field(default_factory=dict)
    region_off: Optional[numpy.ndarray] = None
    region_rows: Optional[numpy.ndarray] = None
    tol: Optional[float] = None      # the tol the pieces were cut with; the default of reduced()

    def __len__(self) -> int:
        return len(self.source)

    def rows_of(self, k: int) -> numpy.ndarray:
        return self.piece_rows[self.piece_off[k]:self.piece_off[k + 1]]

    def pieces_of(self, i: int) -> numpy.ndarray:
        """the indices of the pieces of region i"""
        return numpy.arange(numpy.searchsorted(self.source, i, side='left'), numpy.searchsorted(self.source, i, side='right'))

    def polytopes(self) -> list:
        from .geometry.polytope import Polytope
        return [Polytope(self.rows_of(k)[:, 1:].copy(), self.rows_of(k)[:, :1].copy()) for k in range(len(self))]

    def contains(self, thetas, tol: float = 0.0) -> numpy.ndarray:
        """[n] int64: the first piece with n.theta <= o + tol on every row, or -1.  Host only."""
        n_t = self.piece_rows.shape[1] - 1
        th = numpy.asarray(thetas, dtype=numpy.float64)
        if th.ndim == 1:
            th = th.reshape(1, -1)
        if th.ndim != 2 or th.shape[1] != n_t:
            raise ValueError(f'ExitSets.contains: thetas must be [n, {n_t}], not {list(numpy.shape(thetas))}')
        out = numpy.full(len(th), -1, dtype=numpy.int64)
        if not len(self) or not len(th):
            return out
        chunk = max(1, (1 << 24) // max(1, len(self.piece_rows)))
        for a in range(0, len(th), chunk):
            viol = self.piece_rows[:, 1:] @ th[a:a + chunk].T - self.piece_rows[:, :1]
            inside = numpy.maximum.reduceat(viol, self.piece_off[:-1], axis=0) <= tol
            out[a:a + chunk] = numpy.where(inside.any(axis=0), inside.argmax(axis=0), -1)
        return out

    def reduced(self, tol: Optional[float] = None, device: int = 0) -> 'ExitSets':
        """These exit sets with every piece reduced to its irredundant rows in one device call (geometry.reduce_rows_of):
        a new ExitSets with the same pieces in the same order; source and whole are kept, wide is or-ed with the reduction's, region_off
        and region_rows are unchanged, and stats gains reduce_lps, reduce_ms and rows_removed.  ``tol``: None takes the tol the pieces
        were cut with (1e-8 when unknown).  A piece thinner than tol stays as it is.  This object is not modified."""
        from .geometry.reduce import reduce_rows_of
        tol = (1e-8 if self.tol is None else self.tol) if tol is None else tol
        stats = dict(self.stats, reduce_lps=0, reduce_ms=0.0, rows_removed=0)
        off, rows, wide = self.piece_off.copy(), self.piece_rows.copy(), self.wide.copy()
        if len(self):
            r = reduce_rows_of(self.piece_off, self.piece_rows, self.piece_rows.shape[1] - 1, tol=tol, device=device, who='ExitSets.reduced')
            off, rows, wide = r.row_off, r.rows, wide | (r.wide > 0)
            stats.update(reduce_lps=r.stats['lps'], reduce_ms=r.stats['device_ms'], rows_removed=r.stats['rows_before'] - r.stats['rows_after'])
        elif not (numpy.isfinite(tol) and tol >= 0.0):
            raise ValueError('ExitSets.reduced: tol must be finite and >= 0')
        return ExitSets(n_regions=self.n_regions, piece_off=off, piece_rows=rows, source=self.source.copy(), wide=wide, whole=self.whole.copy(),
                        stats=stats, region_off=self.region_off, region_rows=self.region_rows, tol=self.tol)

    def volumes(self, tol: float = 1e-9, max_simplices=None, device: int = 0) -> ExitVolumes:
        """The volumes of the pieces and of the regions on the device (geometry.volume, with its limits): an ExitVolumes."""
        from . import _lib
        from .geometry.volume import volumes_of_rows
        n_t = self.region_rows.shape[1] - 1
        reg = volumes_of_rows(self.region_off, self.region_rows, n_t, tol=tol, max_simplices=max_simplices, device=device, who='ExitSets.volumes')
        if len(self):
            pv = volumes_of_rows(self.piece_off, self.piece_rows, n_t, tol=tol, max_simplices=max_simplices, device=device, who='ExitSets.volumes')
            piece, piece_status = pv.volume, pv.status
        else:
            piece, piece_status = numpy.zeros(0), numpy.zeros(0, dtype=numpy.int32)
        no_answer = lambda v, st: numpy.where(numpy.isin(st, (_lib.VOL_OK, _lib.VOL_EMPTY)), v, numpy.nan)
        piece, region = no_answer(piece, piece_status), no_answer(reg.volume, reg.status)
        out = numpy.zeros(self.n_regions)
        numpy.add.at(out, self.source, piece)
        with numpy.errstate(invalid='ignore', divide='ignore'):
            share = numpy.where(region > 0.0, out / region, numpy.nan)
            total = float(out.sum() / region.sum()) if region.sum() > 0.0 else float('nan')
        return ExitVolumes(piece=piece, exit=out, region=region, share=share, total_share=total, piece_status=piece_status, region_status=reg.status)


def exit_pieces(row_off, ef_rows, Phi, phi, n_t: int, successors, tol: float = 1e-8, max_pieces: int = 1 << 20, device: int = 0,
                void=(), reduce_rows: bool = False) -> ExitSets:
    """The exit sets on arrays: polytopes of unit rows ef_rows = [o | n] in CSR form by row_off with the maps Phi [R, n_t, n_t], phi
    [R, n_t]; successors[i]: the polytopes whose pulled-back sets are cut out of polytope i (taken ascending, once each).  Steps 2 and 3
    of the module docstring; every LP runs on the device.  ``void``: polytopes known to be empty: they have no piece.
    ``reduce_rows``: the children of every round lose their redundant rows before the row limit is checked (overlap.difference_rounds,
    ``reduce``)."""
    from . import _lib
    t0 = time.perf_counter()
    check_scalars('exit_pieces', n_t, tol)
    if int(max_pieces) < 1:
        raise ValueError('exit_pieces: max_pieces must be >= 1')
    Phi, phi = numpy.ascontiguousarray(Phi, dtype=numpy.float64), numpy.ascontiguousarray(phi, dtype=numpy.float64)
    off, ef, _, R = check_polytopes('exit_pieces', row_off, ef_rows, n_t, extra=map_entries(Phi, phi, n_t), word='maps')
    if len(successors) != R:
        raise ValueError('exit_pieces: successors needs one index list per polytope')
    cutters = []
    for s in successors:
        s = numpy.unique(numpy.asarray(s, dtype=numpy.int64).reshape(-1))
        if len(s) and (s[0] < 0 or s[-1] >= R):
            raise ValueError(f'exit_pieces: successors must name polytopes 0..{R - 1}')
        cutters.append(s.tolist())
    stats = {'rounds': 0, 'items': 0, 'lps': 0, 'pivots': 0, 'wide': 0, 'device_ms': 0.0, 'round_ms': [], 'max_item_rows': 0}
    xs, _, usable, s = feasible_points(off, ef, void, device)
    stats['device_ms'] += s['ms']

    # 2. the rounds of the difference (overlap.difference_rounds) against pulled-back cutters
    def launch(poff, prows, item_source, entries, start):
        return _lib.exit_split(off, ef, Phi, phi, poff, prows, numpy.arange(len(entries)), item_source, [j for j, _ in entries], start, tol, device)

    back = [None, None]      # (source, target) and its pulled-back rows: the items of one source in a round follow each other

    def cutting_rows(i, entry, mask, flag):
        j = entry[0]
        if back[0] != (i, j):
            back[:] = (i, j), pulled_back_rows(ef[off[j]:off[j + 1]], Phi[i], phi[i])
        rows = back[1][mask_rows(mask, len(back[1]))]
        return list(rows[~numpy.isnan(rows[:, 0])])

    reduce = (lambda poff, prows, start: _lib.reduce_rows(poff, prows, start, tol, device)) if reduce_rows else None
    live, stats['round_ms'] = difference_rounds('exit_sets', off, ef, xs, usable, [[(j, None) for j in c] for c in cutters], launch, cutting_rows,
                                                max_pieces, stats, 'items', reduce=reduce)
    # 3. only a piece behind an unbounded or capped run can be empty
    suspects = [(i, k) for i in range(R) for k, (pc, wide) in enumerate(live[i]) if wide and pc is not None]
    if suspects:
        rows = [live[i][k][0] for i, k in suspects]
        _, _, st, s = _lib.merge_regions(numpy.concatenate([[0], numpy.cumsum([len(r) for r in rows])]).astype(numpy.int64), numpy.vstack(rows), device)
        stats['device_ms'] += s['ms']
        gone = {ik for ik, e in zip(suspects, st) if e != 0}
        live = [[p for k, p in enumerate(live[i]) if (i, k) not in gone] for i in range(R)]
    pieces = [ef[off[i]:off[i + 1]] if pc is None else pc for i in range(R) for pc, _ in live[i]]
    source = numpy.asarray([i for i in range(R) for _ in live[i]], dtype=numpy.int64)
    wide = numpy.asarray([w for i in range(R) for _, w in live[i]], dtype=bool)
    whole = numpy.asarray([any(pc is None for pc, _ in live[i]) for i in range(R)], dtype=bool)
    piece_off = numpy.concatenate([[0], numpy.cumsum([len(p) for p in pieces])]).astype(numpy.int64)
    piece_rows = numpy.vstack(pieces) if pieces else numpy.zeros((0, n_t + 1))
    stats['pieces'] = len(pieces)
    stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
    return ExitSets(n_regions=R, piece_off=piece_off, piece_rows=piece_rows, source=source, wide=wide, whole=whole, stats=stats, region_off=off,
                    region_rows=ef, tol=float(tol))


def exit_sets(source, A, B, inputs, c=None, tol: float = 1e-8, graph=None, max_pieces: int = 1 << 20, device: int = 0,
              reduce_rows: bool = False) -> ExitSets:
    """Solution.exit_sets (the module docstring): the states of every region whose next state under the plant theta+ = A theta + B u + c,
    u = x*(theta)[inputs], lies in no region.  ``graph``: the TransitionGraph of the same (A, B, inputs, c, tol); built here when None.
    ``reduce_rows``: as in exit_pieces.  The source is not modified."""
    from .invariance import closed_loop_maps
    from .transition import check_source, transition_graph
    t0 = time.perf_counter()
    A, B, inp, c, n_t = check_source(source, A, B, inputs, c, tol)
    if int(max_pieces) < 1:
        raise ValueError('exit_sets: max_pieces must be >= 1')
    regs = source.critical_regions
    if graph is not None and graph.n_regions != len(regs):
        raise ValueError(f'exit_sets: the graph has {graph.n_regions} regions, the solution {len(regs)}')
    off, rows, void = solution_rows(regs, n_t, 'exit_sets')
    if graph is None:
        graph = transition_graph(source, A, B, inp, c=c, tol=tol, device=device)
    _, _, xlaw = source._stacked()
    Phi, phi = closed_loop_maps(xlaw, A, B, inp, c)
    out = exit_pieces(off, rows, Phi, phi, n_t, [graph.successors(i) for i in range(len(regs))], tol=tol, max_pieces=max_pieces,
                      device=device, void=void, reduce_rows=reduce_rows)
    out.stats['graph_ms'] = float(graph.stats.get('wall_ms', 0.0))
    out.stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
    return out
