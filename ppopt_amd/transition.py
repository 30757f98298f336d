"""The transition graph of an explicit controller in closed loop (Solution.transition_graph).

On region R_i = {n.theta <= o} (unit rows [o | n]) the loop is affine, theta+ = Phi_i theta + phi_i (invariance.closed_loop_maps).  The
transition set of the ordered pair (i, j) is T_ij = {theta in R_i : Phi_i theta + phi_i in R_j}; i = j gives a self loop.

  pulled-back row  a row [o | n] of R_j becomes a.theta <= beta with a = Phi_i^T n, beta = o - n.phi_i, s = |a|.  With
                   s > 1e-12 max(1, max |Phi_i|) (TS_ROW_EPS of csrc/transition.hpp) it enters the LP as the unit row
                   [beta / s | a / s]; otherwise it is constant: beta < -tol empties T_ij (radius -inf, no LP), else the row is dropped.
  radius           r_ij = the Chebyshev radius of the rows of R_i followed by the surviving pulled-back rows of R_j, measured in the
                   source's theta-space.
  edge             i -> j iff r_ij > tol.  An unbounded radius run is an edge with radius +inf (UNBOUNDED); a run stopped at the pivot
                   cap is kept as an edge and flagged UNDECIDED: the graph over-approximates and never drops a possible transition.
  witness          the theta at which the radius run ended: in R_i with slack >= r, and its image in R_j.

Lower-dimensional transitions -- through a facet or a vertex, T_ij of radius <= tol -- are not edges, so every statement about
trajectories (reachable, steps_to, cycles_outside) holds for almost every initial state, not for every one.

Stages: feasible points and boxes of the regions (_lib.merge_regions), the exact boxes of the images (k_transition_boxes), candidate
pairs by _pairs.candidate_pairs: image box and region box meet (image_box_pairs, a host sweep, or with sweep='device' geometry.box_pairs), with
screen='rows' without the candidates that one row of the target separates from the image box (geometry.screen_pairs), one
LP per candidate (k_transition_pairs).
"""
import time
from dataclasses import dataclass, field
from typing import Optional

import numpy

from ._pairs import candidate_pairs, check_pair_indices, check_polytopes, check_region_limits, feasible_points, host_pairs, map_entries
from .region_merge import solution_rows

__all__ = ['TransitionGraph', 'transition_graph', 'transition_pairs', 'image_box_pairs', 'screen_box', 'STATUS', 'NO_EDGE', 'EDGE', 'UNBOUNDED', 'UNDECIDED']

STATUS = ('NO_EDGE', 'EDGE', 'UNBOUNDED', 'UNDECIDED')
NO_EDGE, EDGE, UNBOUNDED, UNDECIDED = range(4)      # the status codes of mpc_transition_pairs


def image_box_pairs(image_box: numpy.ndarray, region_box: numpy.ndarray, usable: numpy.ndarray, tol: float):
    """The directed candidates (i, j), sorted by (i, j), among the usable regions: the image box of i (image_box [R, 2, n_t], lower /
    upper) and the region box of j (region_box [R, 2, n_t]) overlap by more than -tol in every coordinate.  One sweep along the first
    coordinate over both kinds of boxes together; infinite bounds are fine, and a box with a NaN bound in a coordinate is open there."""
    return host_pairs('coordinate', image_box, usable, region_box, usable, -tol)


SCREEN_BOX_SLACK = 1e-9      # the least relative widening of an image box before rows screen it (screen_box)


def screen_box(image_box, tol: float) -> numpy.ndarray:
    """The box the row screen tests the rows of a target against: every bound of the image box moved outwards by
    max(tol, SCREEN_BOX_SLACK) (1 + |bound|); infinite bounds stay, NaN bounds stay (they separate nothing).  The screen is safe only
    against a box that CONTAINS the image.  k_transition_boxes computes the bounds by LPs to about 1e-12 relative, and the image of a
    region under a singular map is flat: where it lies in a facet of its target (a saturated state bound), an upper bound of
    5 + 6e-12 is past the target's row theta_k <= 5 by more than the screen's threshold and a real edge would be dropped (29 of 64,205 on
    the complete config 3).  The sweep before it takes the same boxes as good to tol (its margin is -tol)."""
    box = numpy.asarray(image_box, dtype=numpy.float64)
    with numpy.errstate(invalid='ignore'):
        w = max(float(tol), SCREEN_BOX_SLACK) * (1.0 + numpy.abs(box))
        return numpy.stack([box[:, 0] - w[:, 0], box[:, 1] + w[:, 1]], axis=1)


def transition_pairs(row_off, ef_rows, Phi, phi, n_t: int, tol: float = 1e-8, full_radius: bool = False, pairs=None, device: int = 0,
                     void=(), sweep: str = 'host', screen: str = 'none') -> dict:
    """The pair stage on arrays: polytopes of unit rows ef_rows = [o | n] in CSR form by row_off with the maps Phi [R, n_t, n_t], phi
    [R, n_t].  ``pairs`` = None: image boxes, candidates by image_box_pairs, then one LP per candidate; ``pairs`` = (i, j) arrays: those
    pairs, without the screen.  ``full_radius``: every radius run goes to its optimum (the radius is r_ij and the witness the Chebyshev
    centre) instead of stopping once the radius exceeds tol (the radius is then a lower bound above tol).  ``void``: polytopes known to
    be empty, like the ones the device finds empty: they are no candidates.  ``sweep`` = 'device': the candidates come from
    geometry.box_pairs, the same list as image_box_pairs gives.  ``screen`` = 'rows' (with ``pairs`` None): the candidates that a row of the
    target region separates from the source's image box, widened by screen_box, are dropped before the LPs; stats gains box_candidates,
    screened, screen_ms and the result ``screen_box``, the boxes that were screened.

    Returns a dict: i, j (sorted by (i, j)), radius, status (NO_EDGE, EDGE, UNBOUNDED, UNDECIDED), witness [pairs, n_t], region_status
    [R] (UNDECIDED where the box stage was capped, else 0), image_box, region_box, usable and stats."""
    from . import _lib
    from .geometry.box_pairs import sweep_options
    sweep_options('transition_pairs', sweep, screen)
    Phi, phi = numpy.ascontiguousarray(Phi, dtype=numpy.float64), numpy.ascontiguousarray(phi, dtype=numpy.float64)
    off, ef, _, R = check_polytopes('transition_pairs', row_off, ef_rows, n_t, tol, extra=map_entries(Phi, phi, n_t), word='maps')
    if pairs is not None:
        pa, pb = check_pair_indices('transition_pairs', 'pairs', pairs[0], pairs[1], R)
        o = numpy.lexsort((pb, pa))
        pa, pb = pa[o], pb[o]
    stats = {'box_ms': 0.0, 'pair_ms': 0.0, 'sweep_ms': 0.0, 'candidates': 0, 'lps': 0, 'pivots': 0, 'capped': 0, 'edges': 0, 'box_lps': 0,
             'box_pivots': 0}
    xs, region_box, usable, s = feasible_points(off, ef, void, device)
    stats['box_ms'] += s['ms']
    region_status = numpy.zeros(R, dtype=numpy.int32)
    image_box = None
    screened = []      # the widened image boxes, once the screen has asked for them
    if pairs is None:
        image_box, capped, s = _lib.transition_boxes(off, ef, Phi, phi, xs, device)
        stats['box_ms'] += s['ms']
        stats['box_lps'], stats['box_pivots'] = s['lps'], s['pivots']
        region_status[capped != 0] = UNDECIDED

        def screen_boxes():
            screened.append(screen_box(image_box, tol))
            return None, screened[0]

        pa, pb, swept = candidate_pairs('transition_pairs', 'coordinate', image_box, usable, region_box, usable, -tol, off, ef, screen_boxes, 'b',
                                        sweep, screen, device)
        stats.update(swept)
    stats['candidates'] = len(pa)
    if len(pa):
        radius, st, witness, s = _lib.transition_pairs(off, ef, Phi, phi, xs, pa, pb, full_radius, tol, device)
        stats['pair_ms'] = s['ms']
        for k in ('lps', 'pivots', 'capped'):
            stats[k] = s[k]
    else:
        radius, st, witness = numpy.zeros(0), numpy.zeros(0, dtype=numpy.int32), numpy.zeros((0, n_t))
    stats['edges'] = int(numpy.sum(st != NO_EDGE))
    res = {'i': pa, 'j': pb, 'radius': radius, 'status': st, 'witness': witness, 'region_status': region_status, 'image_box': image_box,
           'region_box': region_box, 'usable': usable, 'stats': stats}
    if screened:
        res['screen_box'] = screened[0]
    return res


def _csr(n: int, src: numpy.ndarray, dst: numpy.ndarray):
    """(indptr, order) of the edges grouped by src, ties by dst"""
    order = numpy.lexsort((dst, src))
    indptr = numpy.concatenate([[0], numpy.cumsum(numpy.bincount(src, minlength=n))]).astype(numpy.int64)
    return indptr, order


@dataclass
class TransitionGraph:
    """The successors of every region in CSR form: region i's are indices[indptr[i]:indptr[i + 1]], ascending; per edge radius, status
    (EDGE, UNBOUNDED: radius +inf, UNDECIDED: the radius run stopped at the pivot cap and the edge is kept) and witness [edges, n_t].
    region_status [n_regions]: UNDECIDED for a region whose image-box run was capped (its box is then the whole space and nothing is
    lost), else 0.  stats: box_ms, pair_ms (device), sweep_ms (host), candidates, lps, pivots, capped, edges.

    An edge is a transition set of radius above tol: transitions through a facet or a vertex are not edges, so reachable, steps_to and
    cycles_outside speak of almost every initial state, not of every one."""
    n_regions: int
    indptr: numpy.ndarray
    indices: numpy.ndarray
    radius: numpy.ndarray
    status: numpy.ndarray
    witness: numpy.ndarray
    region_status: numpy.ndarray
    stats: dict = field(default_factory=dict)
    _pred: Optional[tuple] = field(default=None, repr=False, compare=False)

    @classmethod
    def from_edges(cls, n_regions: int, src, dst, radius=None, status=None, witness=None, region_status=None, stats=None):
        """A graph from an edge list (any order; radius, status and witness follow their edges)."""
        src = numpy.asarray(src, dtype=numpy.int64).reshape(-1)
        dst = numpy.asarray(dst, dtype=numpy.int64).reshape(-1)
        if src.shape != dst.shape or (len(src) and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= n_regions)):
            raise ValueError('TransitionGraph: edges must name regions 0..n_regions - 1')
        indptr, order = _csr(n_regions, src, dst)
        m = len(src)
        radius = numpy.full(m, numpy.nan) if radius is None else numpy.asarray(radius, dtype=numpy.float64)[order]
        status = numpy.full(m, EDGE, dtype=numpy.int32) if status is None else numpy.asarray(status, dtype=numpy.int32)[order]
        witness = numpy.zeros((m, 0)) if witness is None else numpy.asarray(witness, dtype=numpy.float64)[order]
        region_status = numpy.zeros(n_regions, dtype=numpy.int32) if region_status is None else numpy.asarray(region_status, dtype=numpy.int32)
        return cls(int(n_regions), indptr, dst[order], radius, status, witness, region_status, dict(stats or {}))

    def sources(self) -> numpy.ndarray:
        """the source region of every edge"""
        return numpy.repeat(numpy.arange(self.n_regions), numpy.diff(self.indptr))

    def has_edge(self, i: int, j: int) -> bool:
        s = self.successors(i)
        k = numpy.searchsorted(s, j)
        return bool(k < len(s) and s[k] == j)

    def successors(self, i: int) -> numpy.ndarray:
        return self.indices[self.indptr[i]:self.indptr[i + 1]]

    def predecessors(self, i: int) -> numpy.ndarray:
        if self._pred is None:
            src = self.sources()
            indptr, order = _csr(self.n_regions, self.indices, src)
            self._pred = (indptr, src[order])
        return self._pred[1][self._pred[0][i]:self._pred[0][i + 1]]

    def _mask(self, regions, what: str) -> numpy.ndarray:
        idx = numpy.asarray(regions, dtype=numpy.int64).reshape(-1)
        if len(idx) and (idx.min() < 0 or idx.max() >= self.n_regions):
            raise ValueError(f'{what}: regions must lie in 0..{self.n_regions - 1}')
        mask = numpy.zeros(self.n_regions, dtype=bool)
        mask[idx] = True
        return mask

    def _adjacency(self):
        from scipy.sparse import csr_matrix
        return csr_matrix((numpy.ones(len(self.indices), dtype=numpy.int8), self.indices, self.indptr), shape=(self.n_regions, self.n_regions))

    def reachable(self, from_regions) -> numpy.ndarray:
        """The forward closure: the ascending regions some path of edges reaches from ``from_regions``, themselves included."""
        seen = self._mask(from_regions, 'reachable')
        front = numpy.flatnonzero(seen)
        while len(front):
            nxt = numpy.unique(numpy.concatenate([self.successors(i) for i in front]))
            front = nxt[~seen[nxt]]
            seen[front] = True
        return numpy.flatnonzero(seen)

    def steps_to(self, target_regions):
        """(lower, upper) per region, in steps until a trajectory first lies in the target set: lower is the fewest edges to it (inf:
        unreachable), upper the most, through regions outside it; upper is inf where a cycle outside the target (a self loop is one) or a
        region outside the target without successor can come first.  The target set must be closed under successors: ValueError naming
        an edge that leaves it otherwise.  Both bounds are 0 on the target."""
        target = self._mask(target_regions, 'steps_to')
        src = self.sources()
        out = numpy.flatnonzero(target[src] & ~target[self.indices])
        if len(out):
            raise ValueError(f'steps_to: the target set is not closed under successors: the edge {int(src[out[0]])} -> '
                             f'{int(self.indices[out[0]])} leaves it')
        lower, upper = numpy.full(self.n_regions, numpy.inf), numpy.full(self.n_regions, numpy.inf)
        lower[target] = upper[target] = 0.0
        front, d = numpy.flatnonzero(target), 0
        while len(front):
            d += 1
            nxt = numpy.unique(numpy.concatenate([self.predecessors(j) for j in front]))
            front = nxt[numpy.isinf(lower[nxt])]
            lower[front] = d
        # longest paths: a region is settled once every successor is; one on or behind a cycle, or behind a dead end, never is
        pending = numpy.bincount(src[~target[self.indices]], minlength=self.n_regions)
        ready = [int(i) for i in numpy.flatnonzero(~target & (pending == 0) & (numpy.diff(self.indptr) > 0))]
        while ready:
            i = ready.pop()
            upper[i] = 1.0 + float(numpy.max(upper[self.successors(i)]))
            for p in self.predecessors(i).tolist():
                pending[p] -= 1
                if pending[p] == 0:
                    ready.append(p)
        return lower, upper

    def cycles_outside(self, target_regions):
        """The strongly connected components among the regions outside the target set that hold more than one region or a self loop:
        a list of ascending index arrays, ordered by their smallest region."""
        from scipy.sparse.csgraph import connected_components
        outside = numpy.flatnonzero(~self._mask(target_regions, 'cycles_outside'))
        if not len(outside):
            return []
        sub = self._adjacency()[outside][:, outside]
        _, label = connected_components(sub, directed=True, connection='strong')
        loops = sub.diagonal() != 0
        size = numpy.bincount(label)
        keep = numpy.unique(label[(size[label] > 1) | loops])
        comps = [outside[label == c] for c in keep]
        return sorted(comps, key=lambda c: int(c[0]))


def check_source(source, A, B, inputs, c, tol: float):
    """(A, B, inputs, c, n_theta) of a solution transition_graph accepts; ValueError otherwise, before anything reaches the device."""
    from .invariance import _check
    who = 'transition_graph'
    if source.critical_regions and source.is_overlapping:
        raise ValueError(f'{who}: the solution is flagged overlapping: a point may lie in several regions, and which law acts there is '
                         f'chosen by objective; reduce it with remove_overlaps first')
    A, B, inp, c, _, n_t = _check(source, A, B, inputs, c, None, tol, who=who)
    check_region_limits(who, source.critical_regions, n_t)
    return A, B, inp, c, n_t


def transition_graph(source, A, B, inputs, c=None, tol: float = 1e-8, full_radius: bool = False, device: int = 0, sweep: str = 'host',
                     screen: str = 'none') -> TransitionGraph:
    """Solution.transition_graph (the module docstring): which region can follow which under the plant theta+ = A theta + B u + c,
    u = x*(theta)[inputs].  The source is not modified.  ``sweep``, ``screen``: as for transition_pairs; the graph is the same either way."""
    from .invariance import closed_loop_maps
    from .geometry.box_pairs import sweep_options
    sweep_options('transition_graph', sweep, screen)
    t0 = time.perf_counter()
    A, B, inp, c, n_t = check_source(source, A, B, inputs, c, tol)
    off, rows, void = solution_rows(source.critical_regions, n_t, 'transition_graph')
    _, _, xlaw = source._stacked()
    Phi, phi = closed_loop_maps(xlaw, A, B, inp, c)
    res = transition_pairs(off, rows, Phi, phi, n_t, tol=tol, full_radius=full_radius, device=device, void=void, sweep=sweep,
                           screen=screen)
    keep = res['status'] != NO_EDGE
    stats = dict(res['stats'])
    stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
    return TransitionGraph.from_edges(len(off) - 1, res['i'][keep], res['j'][keep], res['radius'][keep], res['status'][keep], res['witness'][keep],
                                      res['region_status'], stats)
