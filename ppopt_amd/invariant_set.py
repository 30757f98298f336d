"""The maximal invariant subset of an explicit controller in closed loop, by backward exit cells (Solution.invariant_set).

On region R_i = {n.theta <= o} (unit rows [o | n]) the loop is affine, theta+ = f_i(theta) = Phi_i theta + phi_i
(invariance.closed_loop_maps).  Omega_0 is the union of the regions.

  E_0        the exit pieces of exit_sets.py, unchanged: the states whose next state lies in no region.
  E_{k+1}    the union over i of R_i n f_i^-1(E_k): the states that leave after exactly k + 2 steps.  First-exit times are unique, so the
             E_k are disjoint by construction and nothing is subtracted between steps.
  Omega_inf  Omega_0 minus every E_k: the states from which the loop stays in the solution for ever.

A CELL of step k + 1 is R_i n f_i^-1(Q) for a cell Q of step k and a predecessor i of Q's source region in the transition graph; no other
pair can have a radius above tol, because R_i n f_i^-1(R_j) already has not.  The items of a step are ordered by parent cell, then by i
ascending; the cells of a step keep item order; the result lists the cells step by step.  Per item (csrc/invariant.hpp, k_pre_cells):

  1. the rows of Q pulled back through (Phi_i, phi_i) with the rule of the transition graph: a constant row with beta < -tol means no
     cell (and no LP), any other constant row is dropped;
  2. the radius of R_i's rows and the pulled-back ones, from region i's feasible point, stopped once it exceeds tol: optimal and not
     above tol means no cell; unbounded or capped keeps the cell and flags it wide;
  3. a kept cell loses its redundant rows by the sequential rule of geometry/reduce.py over the region's rows, then the pulled-back ones.

Every step runs inside one library call (_lib.backward_exits): the cell rows stay on the device from the first step to the last.  The
iteration has converged when a step yields no cell.

Wide cells over-approximate what leaves, so Omega_inf as reported never keeps a state that leaves through a cell of radius above tol.
Parts thinner than tol are not reported, at any step: every statement holds for almost every state.  When the iteration stops early
(max_steps, or a refusal of the library: a reduced cell above 256 rows, max_cells, max_rows_total), the cells of the completed steps are
returned, ``converged`` is False and ``status`` names the reason; a state outside every returned cell then stays for at least
``steps`` + 1 steps.  Disturbances, merging cells back and control-invariant sets are out of scope.
"""
import time
from dataclasses import dataclass, field
from typing import Optional

import numpy

from ._cells import check_cell_call, fill_stats, new_stats
from ._pairs import feasible_points
from .region_merge import mask_rows, solution_rows

__all__ = ['InvariantSet', 'InvariantVolumes', 'invariant_set', 'backward_exit_cells']


@dataclass
class InvariantVolumes:
    """cell [cells]: the volume of every cell; lost_per_step [steps + 1] and lost_per_region [n_regions]: their sums; region [n_regions]:
    the regions' own volumes; invariant [n_regions] = region - lost_per_region; share: the summed invariant volume over the summed region
    volume.  NaN where the volume pass gives no answer (geometry.volume: OVERFLOW, TOO_LARGE, INCONSISTENT, or an unbounded polytope)."""
    cell: numpy.ndarray
    lost_per_step: numpy.ndarray
    lost_per_region: numpy.ndarray
    region: numpy.ndarray
    invariant: numpy.ndarray
    share: float
    cell_status: numpy.ndarray
    region_status: numpy.ndarray


def _inside(off, rows, th, tol):
    """[polytopes, points] bool: n.theta <= o + tol on every row of the polytope"""
    viol = rows[:, 1:] @ th.T - rows[:, :1]
    return numpy.maximum.reduceat(viol, off[:-1], axis=0) <= tol


@dataclass
class InvariantSet:
    """The cells in CSR form, step by step: cell c has the unit rows [o | n] cell_rows[cell_off[c]:cell_off[c + 1]], lies in region
    source[c] and holds states that leave the solution after exactly step[c] + 1 steps; parent[c] is the cell of step[c] - 1 its image
    lies in (-1 at step 0); wide[c]: a radius run on the way to it, or to an ancestor, was unbounded or capped, the cell may hold states
    that stay longer.  steps: the completed steps that yielded cells; converged: the step after them yielded none; status: 'CONVERGED',
    'MAX_STEPS', 'ROWS', 'MAX_CELLS' or 'MAX_ROWS_TOTAL' (the module docstring).  point [cells, n_t]: for the cells of the steps >= 1 the
    point where their radius run ended, NaN at step 0.  stats: items, cells, empty, lps, pivots, wide, cells_per_step, step_ms (device ms
    per step), device_ms, call_ms (the wall time of the library call) and wall_ms.  region_off, region_rows: the regions."""
    n_regions: int
    cell_off: numpy.ndarray
    cell_rows: numpy.ndarray
    source: numpy.ndarray
    step: numpy.ndarray
    parent: numpy.ndarray
    wide: numpy.ndarray
    converged: bool
    steps: int
    stats: dict = field(default_factory=dict)
    region_off: Optional[numpy.ndarray] = None
    region_rows: Optional[numpy.ndarray] = None
    tol: float = 1e-8
    status: str = 'CONVERGED'
    point: Optional[numpy.ndarray] = None

    def __len__(self) -> int:
        return len(self.source)

    def rows_of(self, c: int) -> numpy.ndarray:
        return self.cell_rows[self.cell_off[c]:self.cell_off[c + 1]]

    def cells_of(self, i: int) -> numpy.ndarray:
        """the indices of the cells of region i, in the order of the result"""
        return numpy.flatnonzero(self.source == i)

    def polytopes(self) -> list:
        from .geometry.polytope import Polytope
        return [Polytope(self.rows_of(c)[:, 1:].copy(), self.rows_of(c)[:, :1].copy()) for c in range(len(self))]

    def exit_step(self, thetas, tol: float = 0.0) -> numpy.ndarray:
        """[n] int64: k + 1 for a point in a cell of step k (the first such cell: the earliest exit), 0 for a point in a region and in no
        cell (it stays, as far as the iteration went), -1 for a point outside every region.  Membership is n.theta <= o + tol on every
        row.  Host only."""
        n_t = self.region_rows.shape[1] - 1
        th = numpy.asarray(thetas, dtype=numpy.float64)
        if th.ndim == 1:
            th = th.reshape(1, -1)
        if th.ndim != 2 or th.shape[1] != n_t:
            raise ValueError(f'InvariantSet.exit_step: thetas must be [n, {n_t}], not {list(numpy.shape(thetas))}')
        out = numpy.full(len(th), -1, dtype=numpy.int64)
        if not len(th):
            return out
        chunk = max(1, (1 << 24) // max(1, len(self.region_rows) + len(self.cell_rows)))
        for a in range(0, len(th), chunk):
            part = th[a:a + chunk]
            res = numpy.where(_inside(self.region_off, self.region_rows, part, tol).any(axis=0), 0, -1)
            if len(self):
                inside = _inside(self.cell_off, self.cell_rows, part, tol)
                res = numpy.where((res == 0) & inside.any(axis=0), self.step[inside.argmax(axis=0)] + 1, res)
            out[a:a + chunk] = res
        return out

    def contains(self, thetas, tol: float = 0.0) -> numpy.ndarray:
        """[n] bool: exit_step == 0, the point lies in the invariant subset as far as the iteration went."""
        return self.exit_step(thetas, tol) == 0

    def volumes(self, tol: float = 1e-9, max_simplices=None, device: int = 0) -> InvariantVolumes:
        """The volumes of the cells and of the regions on the device (geometry.volume, with its limits): an InvariantVolumes."""
        from . import _lib
        from .geometry.volume import volumes_of_rows
        n_t = self.region_rows.shape[1] - 1
        who = 'InvariantSet.volumes'
        reg = volumes_of_rows(self.region_off, self.region_rows, n_t, tol=tol, max_simplices=max_simplices, device=device, who=who)
        if len(self):
            cv = volumes_of_rows(self.cell_off, self.cell_rows, n_t, tol=tol, max_simplices=max_simplices, device=device, who=who)
            cell, cell_status = cv.volume, cv.status
        else:
            cell, cell_status = numpy.zeros(0), numpy.zeros(0, dtype=numpy.int32)
        no_answer = lambda v, st: numpy.where(numpy.isin(st, (_lib.VOL_OK, _lib.VOL_EMPTY)), v, numpy.nan)
        cell, region = no_answer(cell, cell_status), no_answer(reg.volume, reg.status)
        per_step, per_region = numpy.zeros(self.steps + 1), numpy.zeros(self.n_regions)
        numpy.add.at(per_step, self.step, cell)
        numpy.add.at(per_region, self.source, cell)
        total = region.sum()
        share = float((total - per_region.sum()) / total) if total > 0.0 else float('nan')
        return InvariantVolumes(cell=cell, lost_per_step=per_step, lost_per_region=per_region, region=region, invariant=region - per_region,
                                share=share, cell_status=cell_status, region_status=reg.status)

    def pieces(self, reduce_rows: bool = False, max_pieces: int = 1 << 20, device: int = 0):
        """Omega_inf itself as convex pieces per region, R_i minus its cells, in the layout of exit_sets.ExitSets (whole[i]: region i has
        no cell that cuts it).  The region difference of the overlap removal (overlap.difference_rounds on k_overlap_split)
        with the cells of the region as cutters, one per round, in cell order.  ``reduce_rows``: as in exit_sets.exit_pieces."""
        from . import _lib
        from .exit_sets import ExitSets
        from .overlap import difference_rounds
        t0 = time.perf_counter()
        R, n_t, tol = self.n_regions, self.region_rows.shape[1] - 1, self.tol
        # regions and cells in one table: difference_rounds names a cutter by its index there; the cells themselves have no piece
        off = numpy.concatenate([self.region_off, self.region_off[-1] + self.cell_off[1:]]).astype(numpy.int64)
        ef = numpy.vstack([self.region_rows, self.cell_rows])
        stats = {'rounds': 0, 'items': 0, 'lps': 0, 'pivots': 0, 'wide': 0, 'device_ms': 0.0, 'round_ms': [], 'max_item_rows': 0}
        xs, _, usable, s = feasible_points(self.region_off, self.region_rows, (), device)
        stats['device_ms'] += s['ms']
        xs = numpy.vstack([xs, numpy.zeros((len(self), n_t))])
        usable = numpy.concatenate([usable, numpy.zeros(len(self), dtype=bool)])
        cutters = [[(R + int(c), None) for c in self.cells_of(i)] for i in range(R)] + [[] for _ in range(len(self))]

        def launch(poff, prows, item_source, entries, start):
            n = len(entries)
            return _lib.overlap_split(off, ef, poff, prows, numpy.arange(n), [j for j, _ in entries], numpy.zeros(n, dtype=numpy.int32), None, start,
                                      tol, device)

        def cutting_rows(i, entry, mask, flag):
            rows = ef[off[entry[0]]:off[entry[0] + 1]]
            return list(rows[mask_rows(mask, len(rows))])

        reduce = (lambda poff, prows, start: _lib.reduce_rows(poff, prows, start, tol, device)) if reduce_rows else None
        live, stats['round_ms'] = difference_rounds('InvariantSet.pieces', off, ef, xs, usable, cutters, launch, cutting_rows, max_pieces, stats,
                                                    'items', reduce=reduce)
        live = live[:R]
        # only a piece behind an unbounded or capped run can be empty
        suspects = [(i, k) for i in range(R) for k, (pc, wide) in enumerate(live[i]) if wide and pc is not None]
        if suspects:
            rows = [live[i][k][0] for i, k in suspects]
            _, _, st, s = _lib.merge_regions(numpy.concatenate([[0], numpy.cumsum([len(r) for r in rows])]).astype(numpy.int64), numpy.vstack(rows),
                                             device)
            stats['device_ms'] += s['ms']
            gone = {ik for ik, e in zip(suspects, st) if e != 0}
            live = [[p for k, p in enumerate(live[i]) if (i, k) not in gone] for i in range(R)]
        pieces = [self.region_rows[self.region_off[i]:self.region_off[i + 1]] if pc is None else pc for i in range(R) for pc, _ in live[i]]
        source = numpy.asarray([i for i in range(R) for _ in live[i]], dtype=numpy.int64)
        wide = numpy.asarray([w for i in range(R) for _, w in live[i]], dtype=bool)
        whole = numpy.asarray([any(pc is None for pc, _ in live[i]) for i in range(R)], dtype=bool)
        piece_off = numpy.concatenate([[0], numpy.cumsum([len(p) for p in pieces])]).astype(numpy.int64)
        piece_rows = numpy.vstack(pieces) if pieces else numpy.zeros((0, n_t + 1))
        stats['pieces'] = len(pieces)
        stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
        return ExitSets(n_regions=R, piece_off=piece_off, piece_rows=piece_rows, source=source, wide=wide, whole=whole, stats=stats,
                        region_off=self.region_off, region_rows=self.region_rows, tol=float(tol))


def backward_exit_cells(row_off, ef_rows, Phi, phi, n_t: int, predecessors, cell_off, cell_rows, cell_source, tol: float = 1e-8,
                        max_steps: int = 64, max_cells: int = 1 << 20, device: int = 0, max_rows_total: Optional[int] = None,
                        void=()) -> InvariantSet:
    """The backward exit cells on arrays: polytopes of unit rows ef_rows = [o | n] in CSR form by row_off with the maps Phi [R, n_t, n_t],
    phi [R, n_t]; predecessors[j]: the polytopes whose image can meet polytope j (taken ascending, once each); cell_off, cell_rows,
    cell_source: the cells of step 0, each inside polytope cell_source[c].  The steps of the module docstring; every LP runs on the
    device, in one library call.  max_cells and max_rows_total (None: 2^26 // (n_t + 1)) bound the cells and the rows of all steps, step
    0 included; ``void``: polytopes known to be empty: they precede nothing.  Every ValueError is raised before the library is touched."""
    from . import _lib
    t0 = time.perf_counter()
    off, ef, Phi, phi, pred_off, pred_idx, coff, crow, csrc, max_rows_total = check_cell_call(
        'backward_exit_cells', row_off, ef_rows, Phi, phi, n_t, 'predecessors', predecessors, cell_off, cell_rows, 'cell_source', 'one source',
        cell_source, tol, max_steps, max_cells, max_rows_total, void)
    R = len(off) - 1
    stats = new_stats(len(csrc))
    if len(csrc) == 0 or int(max_steps) == 0:
        stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
        done = len(csrc) == 0
        return InvariantSet(n_regions=R, cell_off=coff, cell_rows=crow, source=csrc, step=numpy.zeros(len(csrc), dtype=numpy.int64),
                            parent=numpy.full(len(csrc), -1, dtype=numpy.int64), wide=numpy.zeros(len(csrc), dtype=bool), converged=done, steps=0,
                            stats=stats, region_off=off, region_rows=ef, tol=float(tol), status='CONVERGED' if done else 'MAX_STEPS',
                            point=numpy.full((len(csrc), n_t), numpy.nan))
    xs, _, _, s = _lib.merge_regions(off, ef, device)
    stats['device_ms'] += s['ms']
    xs = numpy.where(numpy.isfinite(xs), xs, 0.0)
    t1 = time.perf_counter()
    r = _lib.backward_exits(off, ef, Phi, phi, xs, pred_off, pred_idx, coff, crow, csrc, tol, int(max_steps), int(max_cells), int(max_rows_total),
                            device)
    fill_stats(stats, r, max_steps, t1, t0)
    return InvariantSet(n_regions=R, cell_off=r['cell_off'], cell_rows=r['cell_rows'], source=r['source'], step=r['step'], parent=r['parent'],
                        wide=r['wide'], converged=r['converged'], steps=r['steps'], stats=stats, region_off=off, region_rows=ef, tol=float(tol),
                        status=_lib.BACKWARD_STATUS[r['status']], point=r['point'])


def invariant_set(source, A, B, inputs, c=None, tol: float = 1e-8, graph=None, exits=None, max_steps: int = 64, max_cells: int = 1 << 20,
                  reduce_rows: bool = True, device: int = 0) -> InvariantSet:
    """Solution.invariant_set (the module docstring): the states from which the loop under the plant theta+ = A theta + B u + c,
    u = x*(theta)[inputs], leaves the solution, as cells by the step at which they leave; what no cell holds stays.  ``graph``: the
    TransitionGraph and ``exits``: the ExitSets of the same (A, B, inputs, c, tol); each is built here when None, the exit sets with
    ``reduce_rows`` (on by default: the rows of a cell are pulled back at every step, so rows that bound nothing cost at every step).
    Refusals as for transition_graph.  The source is not modified."""
    from .exit_sets import exit_sets
    from .invariance import closed_loop_maps
    from .transition import check_source, transition_graph
    t0 = time.perf_counter()
    A, B, inp, c, n_t = check_source(source, A, B, inputs, c, tol)
    if int(max_steps) < 0:
        raise ValueError('invariant_set: max_steps must be >= 0')
    if int(max_cells) < 1:
        raise ValueError('invariant_set: max_cells must be >= 1')
    regs = source.critical_regions
    if graph is not None and graph.n_regions != len(regs):
        raise ValueError(f'invariant_set: the graph has {graph.n_regions} regions, the solution {len(regs)}')
    if exits is not None and exits.n_regions != len(regs):
        raise ValueError(f'invariant_set: the exit sets have {exits.n_regions} regions, the solution {len(regs)}')
    off, rows, void = solution_rows(regs, n_t, 'invariant_set')
    if graph is None:
        graph = transition_graph(source, A, B, inp, c=c, tol=tol, device=device)
    if exits is None:
        exits = exit_sets(source, A, B, inp, c=c, tol=tol, graph=graph, max_pieces=max_cells, device=device, reduce_rows=reduce_rows)
    _, _, xlaw = source._stacked()
    Phi, phi = closed_loop_maps(xlaw, A, B, inp, c)
    out = backward_exit_cells(off, rows, Phi, phi, n_t, [graph.predecessors(j) for j in range(len(regs))], exits.piece_off, exits.piece_rows,
                              exits.source, tol=tol, max_steps=max_steps, max_cells=max_cells, device=device, void=void)
    out.wide = out.wide | numpy.asarray(exits.wide, dtype=bool)[_root(out.parent)] if len(out) else out.wide
    out.stats['graph_ms'] = float(graph.stats.get('wall_ms', 0.0))
    out.stats['exit_ms'] = float(exits.stats.get('wall_ms', 0.0))
    out.stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
    return out


def _root(parent: numpy.ndarray) -> numpy.ndarray:
    """the cell of step 0 every cell descends from (parents come before their children)"""
    root = numpy.arange(len(parent))
    for c in range(len(parent)):
        if parent[c] >= 0:
            root[c] = root[parent[c]]
    return root
