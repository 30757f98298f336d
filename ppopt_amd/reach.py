"""The forward cells of an explicit controller in closed loop: k-step maps and reachable sets (Solution.reach_cells).

On region R_i = {n.theta <= o} (unit rows [o | n]) the loop is affine, theta+ = f_i(theta) = Phi_i theta + phi_i
(invariance.closed_loop_maps).  The backward side (exit_sets.py, invariant_set.py) asks which states leave; this module follows SETS of
initial states forward.

A CELL of step k is a set Q of INITIAL states theta_0, stored as unit rows over theta_0, with

  region(Q)  the region i_k the state is in at step k,
  (G, g)     the composed map: theta_k = G theta_0 + g on Q,
  parent     the cell of step k - 1 it was cut from; the region sequence i_0 .. i_k is read off the parents.

Cells live in initial-state coordinates on purpose.  Pushing a cell through f_i and intersecting the image with the regions needs
Phi_i^-1, and singular closed-loop maps occur; and under a contracting loop every image gets thinner than tol after a few dozen steps, so
the "radius above tol" rule would drop the whole bundle of trajectories.  Here a map is only ever pulled back through, and "thin" means
thin in X_0: every statement holds for almost every initial state, whatever the loop contracts or expands.

Step 0 is given: cells inside their regions with (G, g) = (I, 0) and an interior point each.  The NEXT MAP of a cell Q with region i is
P = Phi_i G, s = Phi_i g + phi_i, every entry one sum over t ascending from 0.0 of plain IEEE products.  Step k + 1 has one item (Q, j) for
every cell Q of step k and every j in successors(region(Q)), ordered by parent cell, then by j ascending; the cells keep item order; the
result lists the cells step by step.  Per item (csrc/forward.hpp, k_fwd_cells):

  1. the rows of R_j pulled back through (P, s) with the rule of the transition graph: a constant row with beta < -tol means no cell (and
     no LP), any other constant row is dropped;
  2. the radius of Q's rows and the pulled-back ones, from Q's point, stopped once it exceeds tol: optimal and not above tol means no
     cell; unbounded or capped keeps the cell and flags it wide, as is every descendant;
  3. a kept cell loses its redundant rows by the sequential rule of geometry/reduce.py over Q's rows, then the pulled-back ones.

The new cell has the kept rows, region j, the map (P, s), the point where the radius run ended, and its parent.  Every step runs inside
one library call (_lib.forward_cells): rows and maps stay on the device from the first step to the last.

status: 'DONE' (max_steps steps were run), 'EMPTY' (a step yielded no cell: every trajectory has left), 'ROWS' (a reduced cell keeps
more than 256 rows), 'MAX_CELLS', 'MAX_ROWS_TOTAL'; after the last three the cells of the completed steps are returned.

If the regions do not overlap, the cells of one step are disjoint up to sets thinner than tol and their union is the states of X_0 still
inside after k steps.  Disturbances, the part of a cell that leaves as pieces, merging cells, and mixed-integer or overlapping sources
are out of scope.
"""
import time
from dataclasses import dataclass, field
from typing import Optional

import numpy

from ._cells import check_cell_call, fill_stats, new_stats
from .invariant_set import _inside
from .region_merge import MAX_ROWS, solution_rows

__all__ = ['ForwardCells', 'ForwardVolumes', 'forward_cells', 'reach_cells']

MAX_COND = 1e12      # images(): a map with a larger condition number gets no H-representation


@dataclass
class ForwardVolumes:
    """cell [cells]: the volume of every cell (in X_0); per_step [steps + 1]: the volume still inside after k steps; per_root
    [cells of step 0, steps + 1]: the same per cell of step 0.  NaN where the volume pass gives no answer (geometry.volume: OVERFLOW,
    TOO_LARGE, INCONSISTENT, or an unbounded polytope)."""
    cell: numpy.ndarray
    per_step: numpy.ndarray
    per_root: numpy.ndarray
    cell_status: numpy.ndarray


@dataclass
class Entering:
    """cell, target [pairs]: the (cell, target) pairs whose {theta_0 in Q : G theta_0 + g in T} has a radius above tol, sorted by cell;
    first_step [targets]: the first step at which some cell enters the target, -1 when none does; witness [pairs, n_t]: an initial
    state of each pair.  stats: those of the transition_pairs call."""
    cell: numpy.ndarray
    target: numpy.ndarray
    first_step: numpy.ndarray
    witness: numpy.ndarray
    stats: dict = field(default_factory=dict)

    def cells_of(self, t: int) -> numpy.ndarray:
        """the cells that enter target t"""
        return self.cell[self.target == t]


@dataclass
class ForwardCells:
    """The cells in CSR form, step by step: cell c has the unit rows [o | n] cell_rows[cell_off[c]:cell_off[c + 1]] over theta_0; the
    state is in region[c] at step[c], where theta_k = G[c] theta_0 + g[c]; parent[c] is the cell of step[c] - 1 it was cut from (-1 at
    step 0); wide[c]: its radius run, or an ancestor's, was unbounded or capped; point [cells, n_t]: a point of the cell (where its
    radius run ended).  steps: the completed steps; status: the module docstring.  stats: items, cells, empty, lps, pivots, wide,
    cells_per_step, step_ms (device ms per step), device_ms, call_ms and wall_ms.  region_off, region_rows: the regions."""
    n_regions: int
    cell_off: numpy.ndarray
    cell_rows: numpy.ndarray
    region: numpy.ndarray
    step: numpy.ndarray
    parent: numpy.ndarray
    G: numpy.ndarray
    g: numpy.ndarray
    wide: numpy.ndarray
    point: numpy.ndarray
    status: str = 'DONE'
    steps: int = 0
    stats: dict = field(default_factory=dict)
    region_off: Optional[numpy.ndarray] = None
    region_rows: Optional[numpy.ndarray] = None
    tol: float = 1e-8

    def __len__(self) -> int:
        return len(self.region)

    @property
    def n_t(self) -> int:
        return self.cell_rows.shape[1] - 1

    def rows_of(self, c: int) -> numpy.ndarray:
        return self.cell_rows[self.cell_off[c]:self.cell_off[c + 1]]

    def cells_at(self, k: int) -> numpy.ndarray:
        """the indices of the cells of step k, in the order of the result"""
        return numpy.flatnonzero(self.step == int(k))

    def itinerary(self, c: int) -> list:
        """the regions i_0 .. i_k the states of cell c pass through, read off the parents"""
        c = int(c)
        if not 0 <= c < len(self):
            raise ValueError(f'ForwardCells.itinerary: cell {c} is outside 0..{len(self) - 1}')
        out = []
        while c >= 0:
            out.append(int(self.region[c]))
            c = int(self.parent[c])
        return out[::-1]

    def _points(self, who, thetas):
        th = numpy.asarray(thetas, dtype=numpy.float64)
        if th.ndim == 1:
            th = th.reshape(1, -1)
        if th.ndim != 2 or th.shape[1] != self.n_t:
            raise ValueError(f'ForwardCells.{who}: thetas must be [n, {self.n_t}], not {list(numpy.shape(thetas))}')
        return th

    def locate(self, thetas, k: int, tol: float = 0.0) -> numpy.ndarray:
        """[n] int64: the first cell of step k that holds each initial state (n.theta <= o + tol on every row), -1 where none does: the
        state has left before step k, or lies in a part thinner than tol.  Host only."""
        th = self._points('locate', thetas)
        at = self.cells_at(k)
        out = numpy.full(len(th), -1, dtype=numpy.int64)
        if not len(at) or not len(th):
            return out
        lo, hi = int(self.cell_off[at[0]]), int(self.cell_off[at[-1] + 1])      # the cells of a step are contiguous
        off, rows = self.cell_off[at[0]:at[-1] + 2] - lo, self.cell_rows[lo:hi]
        chunk = max(1, (1 << 24) // max(1, len(rows)))
        for a in range(0, len(th), chunk):
            inside = _inside(off, rows, th[a:a + chunk], tol)
            out[a:a + chunk] = numpy.where(inside.any(axis=0), at[inside.argmax(axis=0)], -1)
        return out

    def state_at(self, thetas, k: int, tol: float = 0.0) -> numpy.ndarray:
        """[n, n_t]: theta_k = G theta_0 + g with the map of the cell locate finds; NaN rows where it finds none."""
        th = self._points('state_at', thetas)
        c = self.locate(th, k, tol)
        out = numpy.full(th.shape, numpy.nan)
        ok = c >= 0
        out[ok] = numpy.einsum('ktl,kl->kt', self.G[c[ok]], th[ok]) + self.g[c[ok]]
        return out

    def roots(self) -> numpy.ndarray:
        """the cell of step 0 every cell descends from (parents come before their children)"""
        root = numpy.arange(len(self))
        for c in range(len(self)):
            if self.parent[c] >= 0:
                root[c] = root[self.parent[c]]
        return root

    def volumes(self, tol: float = 1e-9, max_simplices=None, device: int = 0) -> ForwardVolumes:
        """The volume of X_0 still inside after every step, in all and per cell of step 0, on the device (geometry.volume, with its
        limits): a ForwardVolumes."""
        from . import _lib
        from .geometry.volume import volumes_of_rows
        n0 = int(numpy.sum(self.step == 0))
        if not len(self):
            return ForwardVolumes(cell=numpy.zeros(0), per_step=numpy.zeros(self.steps + 1), per_root=numpy.zeros((0, self.steps + 1)),
                                  cell_status=numpy.zeros(0, dtype=numpy.int32))
        cv = volumes_of_rows(self.cell_off, self.cell_rows, self.n_t, tol=tol, max_simplices=max_simplices, device=device, who='ForwardCells.volumes')
        cell = numpy.where(numpy.isin(cv.status, (_lib.VOL_OK, _lib.VOL_EMPTY)), cv.volume, numpy.nan)
        per_step, per_root = numpy.zeros(self.steps + 1), numpy.zeros((n0, self.steps + 1))
        numpy.add.at(per_step, self.step, cell)
        numpy.add.at(per_root, (self.roots(), self.step), cell)
        return ForwardVolumes(cell=cell, per_step=per_step, per_root=per_root, cell_status=cv.status)

    def image_vertices(self, k: int, tol: float = 1e-9, device: int = 0) -> list:
        """The images at step k of the cells of step k as vertex lists: per cell [v, n_t], the vertices of the cell
        (geometry.polytope_vertices on the device) mapped through (G, g); valid for a singular G too, where the image is flat.  None
        for a cell the vertex pass does not finish (unbounded, not pointed, empty, overflow)."""
        from .geometry import vertices as vx
        at = self.cells_at(k)
        if not len(at):
            return []
        lo, hi = int(self.cell_off[at[0]]), int(self.cell_off[at[-1] + 1])
        res = vx.vertices_of_rows(self.cell_off[at[0]:at[-1] + 2] - lo, self.cell_rows[lo:hi], self.n_t, tol=tol, device=device,
                                  who='ForwardCells.image_vertices')
        return [res.of(n) @ self.G[c].T + self.g[c] if res.status[n] == vx.OK else None for n, c in enumerate(at)]

    def images(self, k: int) -> list:
        """The images at step k of the cells of step k as unit rows [o | n] over theta_k, formed on the host where cond(G) <= 1e12:
        n.theta_0 <= o with theta_0 = G^-1 (theta_k - g) is (G^-T n).theta_k <= o + (G^-T n).g.  None for the other cells (their images
        are flat or nearly so: image_vertices)."""
        out = []
        for c in self.cells_at(k):
            G = self.G[c]
            if not numpy.all(numpy.isfinite(G)) or numpy.linalg.cond(G) > MAX_COND:
                out.append(None)
                continue
            rows = self.rows_of(c)
            a = numpy.linalg.solve(G.T, rows[:, 1:].T).T
            beta = rows[:, 0] + a @ self.g[c]
            s = numpy.linalg.norm(a, axis=1)
            out.append(numpy.column_stack([beta / s, a / s[:, None]]))
        return out

    def entering(self, targets, tol: Optional[float] = None, device: int = 0) -> Entering:
        """Which cells enter which target: the pairs (cell Q, target T) whose {theta_0 in Q : G theta_0 + g in T} has a Chebyshev radius
        above tol (None: the tolerance of the cells), in one transition_pairs call over cells and targets with the cells' own maps.
        ``targets``: Polytopes or arrays of unit rows [o | n], 1..256 rows each.  With an unsafe set as target, first_step < 0 says no
        trajectory of positive measure enters it within the steps run; with a goal set, the cells that hit are the ones that arrive."""
        from .geometry.polytope import Polytope
        from .geometry.reduce import polytope_unit_rows
        from .transition import NO_EDGE, transition_pairs
        who = 'ForwardCells.entering'
        n_t, nc = self.n_t, len(self)
        tlist = [targets] if isinstance(targets, (Polytope, numpy.ndarray)) else list(targets)
        trows = [polytope_unit_rows(who, t) if isinstance(t, Polytope) else numpy.asarray(t, dtype=numpy.float64).reshape(-1, n_t + 1) for t in tlist]
        if not trows:
            raise ValueError(f'{who}: no targets')
        tol = self.tol if tol is None else float(tol)
        first = numpy.full(len(trows), -1, dtype=numpy.int64)
        if nc == 0:
            return Entering(cell=numpy.zeros(0, dtype=numpy.int64), target=numpy.zeros(0, dtype=numpy.int64), first_step=first,
                            witness=numpy.zeros((0, n_t)))
        off = numpy.concatenate([self.cell_off, self.cell_off[-1] + numpy.cumsum([len(r) for r in trows])]).astype(numpy.int64)
        rows = numpy.vstack([self.cell_rows] + trows)
        Phi = numpy.concatenate([self.G, numpy.tile(numpy.eye(n_t), (len(trows), 1, 1))])
        phi = numpy.concatenate([self.g, numpy.zeros((len(trows), n_t))])
        pa = numpy.repeat(numpy.arange(nc), len(trows))
        pb = nc + numpy.tile(numpy.arange(len(trows)), nc)
        res = transition_pairs(off, rows, Phi, phi, n_t, tol=tol, pairs=(pa, pb), device=device)
        hit = res['status'] != NO_EDGE
        cell, target = res['i'][hit].astype(numpy.int64), res['j'][hit].astype(numpy.int64) - nc
        for t in range(len(trows)):
            if numpy.any(target == t):
                first[t] = int(self.step[cell[target == t]].min())
        return Entering(cell=cell, target=target, first_step=first, witness=res['witness'][hit], stats=dict(res['stats']))

    def polytopes(self) -> list:
        from .geometry.polytope import Polytope
        return [Polytope(self.rows_of(c)[:, 1:].copy(), self.rows_of(c)[:, :1].copy()) for c in range(len(self))]


def forward_cells(row_off, ef_rows, Phi, phi, n_t: int, successors, cell_off, cell_rows, cell_region, cell_point=None, tol: float = 1e-8,
                  max_steps: int = 8, max_cells: int = 1 << 20, max_rows_total: Optional[int] = None, device: int = 0) -> ForwardCells:
    """The forward cells on arrays: polytopes of unit rows ef_rows = [o | n] in CSR form by row_off with the maps Phi [R, n_t, n_t], phi
    [R, n_t]; successors[i]: the polytopes the image of polytope i can meet (taken ascending, once each); cell_off, cell_rows, cell_region:
    the cells of step 0, each inside polytope cell_region[c]; cell_point [cells, n_t]: a point of each (None: a feasible point found on
    the device).  The steps of the module docstring; every LP runs on the device, in one library call.  max_cells and max_rows_total
    (None: 2^26 // (n_t + 1)) bound the cells and the rows of all steps, step 0 included.  Every ValueError is raised before the library
    is touched."""
    t0 = time.perf_counter()
    who = 'forward_cells'
    off, ef, Phi, phi, succ_off, succ_idx, coff, crow, creg, max_rows_total = check_cell_call(
        who, row_off, ef_rows, Phi, phi, n_t, 'successors', successors, cell_off, cell_rows, 'cell_region', 'one region', cell_region, tol, max_steps,
        max_cells, max_rows_total)
    R, n0 = len(off) - 1, len(creg)
    cpt = None
    if cell_point is not None:
        cpt = numpy.ascontiguousarray(cell_point, dtype=numpy.float64)
        if cpt.shape != (n0, n_t) or not numpy.all(numpy.isfinite(cpt)):
            raise ValueError(f'{who}: cell_point must be a finite [{n0}, {n_t}] array')
    stats = new_stats(n0)
    if n0 == 0 or int(max_steps) == 0:
        stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
        return ForwardCells(n_regions=R, cell_off=coff, cell_rows=crow, region=creg, step=numpy.zeros(n0, dtype=numpy.int64),
                            parent=numpy.full(n0, -1, dtype=numpy.int64), G=numpy.tile(numpy.eye(n_t), (n0, 1, 1)), g=numpy.zeros((n0, n_t)),
                            wide=numpy.zeros(n0, dtype=bool), point=numpy.full((n0, n_t), numpy.nan) if cpt is None else cpt,
                            status='EMPTY' if n0 == 0 else 'DONE', steps=0, stats=stats, region_off=off, region_rows=ef, tol=float(tol))
    from . import _lib
    if cpt is None:
        cpt, _, _, s = _lib.merge_regions(coff, crow, device)
        stats['device_ms'] += s['ms']
        cpt = numpy.where(numpy.isfinite(cpt), cpt, 0.0)
    t1 = time.perf_counter()
    r = _lib.forward_cells(off, ef, Phi, phi, succ_off, succ_idx, coff, crow, creg, cpt, tol, int(max_steps), int(max_cells), int(max_rows_total),
                           device)
    fill_stats(stats, r, max_steps, t1, t0)
    return ForwardCells(n_regions=R, cell_off=r['cell_off'], cell_rows=r['cell_rows'], region=r['region'], step=r['step'], parent=r['parent'],
                        G=r['G'], g=r['g'], wide=r['wide'], point=r['point'], status=_lib.FORWARD_STATUS[r['status']], steps=r['steps'],
                        stats=stats, region_off=off, region_rows=ef, tol=float(tol))


def initial_cells(row_off, ef_rows, n_t: int, pieces, tol: float, void=(), device: int = 0):
    """(cell_off, cell_rows, cell_region, cell_point) of step 0 from a list of pieces given as unit rows: every piece n region of radius
    above tol, in piece-then-region order, without its redundant rows.  One transition_pairs call under identity maps over pieces and
    regions, then one reduce_rows_of call started at the witnesses."""
    from .geometry.reduce import reduce_rows_of
    from .transition import NO_EDGE, transition_pairs
    R, P = len(row_off) - 1, len(pieces)
    ends = numpy.cumsum([len(p) for p in pieces])
    off = numpy.concatenate([[0], ends, ends[-1] + row_off[1:]]).astype(numpy.int64)
    rows = numpy.vstack(list(pieces) + [ef_rows])
    live = numpy.setdiff1d(numpy.arange(R), numpy.asarray(list(void), dtype=numpy.int64))
    pa, pb = numpy.repeat(numpy.arange(P), len(live)), P + numpy.tile(live, P)
    res = transition_pairs(off, rows, numpy.tile(numpy.eye(n_t), (P + R, 1, 1)), numpy.zeros((P + R, n_t)), n_t, tol=tol, pairs=(pa, pb),
                           device=device)
    hit = res['status'] != NO_EDGE
    if not hit.any():
        return numpy.zeros(1, dtype=numpy.int64), numpy.zeros((0, n_t + 1)), numpy.zeros(0, dtype=numpy.int64), numpy.zeros((0, n_t))
    pi, ri = res['i'][hit], res['j'][hit] - P
    both = [numpy.vstack([pieces[p], ef_rows[row_off[i]:row_off[i + 1]]]) for p, i in zip(pi, ri)]
    boff = numpy.concatenate([[0], numpy.cumsum([len(b) for b in both])]).astype(numpy.int64)
    red = reduce_rows_of(boff, numpy.vstack(both), n_t, tol=tol, start=res['witness'][hit], device=device, who='reach_cells')
    return red.row_off, red.rows, ri.astype(numpy.int64), red.point


def reach_cells(source, A, B, inputs, c=None, initial=None, steps: int = 8, tol: float = 1e-8, graph=None, max_cells: int = 1 << 20,
                max_rows_total: Optional[int] = None, device: int = 0) -> ForwardCells:
    """Solution.reach_cells (the module docstring): where the states of ``initial`` are after 1 .. ``steps`` steps of the loop under the
    plant theta+ = A theta + B u + c, u = x*(theta)[inputs], as cells of initial states with their region sequences and k-step maps.
    ``initial`` = None: step 0 is the regions themselves; a Polytope or a list of them: every piece n region of radius above tol, in
    piece-then-region order.  ``graph``: the TransitionGraph of the same (A, B, inputs, c, tol), built here when None.  Refusals as for
    transition_graph.  The source is not modified."""
    from .geometry.polytope import Polytope
    from .geometry.reduce import polytope_unit_rows
    from .invariance import closed_loop_maps
    from .transition import check_source, transition_graph
    t0 = time.perf_counter()
    who = 'reach_cells'
    A, B, inp, c, n_t = check_source(source, A, B, inputs, c, tol)
    if int(steps) < 0:
        raise ValueError(f'{who}: steps must be >= 0')
    if int(max_cells) < 1:
        raise ValueError(f'{who}: max_cells must be >= 1')
    regs = source.critical_regions
    if graph is not None and graph.n_regions != len(regs):
        raise ValueError(f'{who}: the graph has {graph.n_regions} regions, the solution {len(regs)}')
    pieces = None
    if initial is not None:
        plist = [initial] if isinstance(initial, Polytope) else list(initial)
        if not plist or not all(isinstance(p, Polytope) for p in plist):
            raise ValueError(f'{who}: initial must be a Polytope or a non-empty list of them')
        pieces = [polytope_unit_rows(who, p) for p in plist]
        if any(p.shape[1] != n_t + 1 for p in pieces) or any(not 1 <= len(p) <= MAX_ROWS for p in pieces):
            raise ValueError(f'{who}: every initial polytope needs n_theta = {n_t} and 1..{MAX_ROWS} rows')
    off, rows, void = solution_rows(regs, n_t, who)
    if graph is None:
        graph = transition_graph(source, A, B, inp, c=c, tol=tol, device=device)
    _, _, xlaw = source._stacked()
    Phi, phi = closed_loop_maps(xlaw, A, B, inp, c)
    if pieces is None:
        live = numpy.setdiff1d(numpy.arange(len(regs)), numpy.asarray(void, dtype=numpy.int64))
        coff = numpy.concatenate([[0], numpy.cumsum(numpy.diff(off)[live])]).astype(numpy.int64)
        crow = numpy.vstack([rows[off[i]:off[i + 1]] for i in live]) if len(live) else numpy.zeros((0, n_t + 1))
        creg, cpt = live.astype(numpy.int64), None
    else:
        coff, crow, creg, cpt = initial_cells(off, rows, n_t, pieces, tol, void=void, device=device)
    out = forward_cells(off, rows, Phi, phi, n_t, [graph.successors(i) for i in range(len(regs))], coff, crow, creg, cell_point=cpt, tol=tol,
                        max_steps=steps, max_cells=max_cells, max_rows_total=max_rows_total, device=device)
    out.stats['graph_ms'] = float(graph.stats.get('wall_ms', 0.0))
    out.stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
    return out
