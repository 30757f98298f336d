"""Solution: the program plus the list of critical regions (reference: solution.py:15-199)."""
import time
from dataclasses import dataclass, field
from typing import List, Optional

import numpy

from .critical_region import CriticalRegion


@dataclass
class SampleCheck:
    """Report of Solution.sample_check.  Global part: points drawn uniformly from the parameter set; per-region part: points drawn
    uniformly inside every full-dimensional region."""
    n_samples: int                  # points of the parameter set
    n_feasible: int                 # ... where the program is feasible
    n_uncovered: int                # feasible, but no region located
    n_wrong: int                    # located, but the located law is not optimal (objective gap or a violated row)
    n_spurious: int                 # located where the program is infeasible
    n_spurious_bad: int             # ... and the law violates a program row by more than tol
    covered_fraction: float         # located share of the feasible points
    max_obj_gap: float              # largest |obj(x_r) - obj*| / (1 + |obj*|) over located feasible points
    max_x_err: Optional[float]      # QPs: largest |x_r - x*|
    uncovered_points: numpy.ndarray = field(repr=False)    # [<= 1000, n_theta]
    n_regions_sampled: int = 0
    n_regions_not_sampled: int = 0  # radius <= 1e-8, more than 256 rows, or no Chebyshev centre
    failing_regions: List[int] = field(default_factory=list)
    seconds: float = 0.0

    @property
    def ok(self) -> bool:
        return self.n_uncovered == 0 and self.n_wrong == 0 and self.n_spurious_bad == 0 and not self.failing_regions


class Solution:
    # Batched point location walks through adjacent regions (csrc/locate.hpp, k_locate_walk) instead of scanning the region
    # list when the solution is complete, has at least this many regions, is not overlapping and came from the device (facet
    # information per row); ``use_walk = False`` forces the scan.
    WALK_MIN_REGIONS = 2048
    use_walk = True
    # the regions cover the whole feasible parameter set (set by the solvers that run to completion): the walk is only used
    # then -- in a partial solution most walks end at a missing neighbour
    is_complete = False
    # set on the result of merge_regions (region_merge.build_merged_solution): source, outputs, members, stats
    merge_info = None
    # set on the result of remove_overlaps (overlap.build_reduced_solution): source, sources, verdict_counts, vanished, stats
    overlap_info = None
    # set on the result of reduce_rows (geometry.reduce.reduce_solution): source, kept, status, wide, stats
    reduce_info = None

    def __init__(self, program, critical_regions: List[CriticalRegion], is_overlapping: bool = False,
                 point_location_tolerance: float = 1e-5):
        self.program = program
        self.critical_regions = critical_regions
        self.is_overlapping = is_overlapping
        self.point_location_tolerance = point_location_tolerance
        self.overlap_info = None

    def add_region(self, region: CriticalRegion) -> None:
        self.critical_regions.append(region)

    def get_region(self, theta_point: numpy.ndarray) -> Optional[CriticalRegion]:
        """First containing region, or the containing region with the lowest objective when regions may overlap
        (solution.py:60-112)."""
        tol = self.point_location_tolerance
        if not self.is_overlapping:
            for cr in self.critical_regions:
                if cr.is_inside(theta_point, tol):
                    return cr
            return None
        best, best_obj = None, float('inf')
        for cr in self.critical_regions:
            if cr.is_inside(theta_point, tol):
                obj = self.program.evaluate_objective(cr.evaluate(theta_point), theta_point)
                if obj <= best_obj:
                    best, best_obj = cr, obj
        return best

    def evaluate(self, theta_point: numpy.ndarray) -> Optional[numpy.ndarray]:
        cr = self.get_region(theta_point)
        return None if cr is None else cr.evaluate(theta_point)

    def _refuse_merged(self, what: str) -> None:
        if self.merge_info is not None:
            raise ValueError(f'{what} needs the full law and the multipliers, which a merged solution does not keep: verify the source '
                             f'(merge_info["source"]) instead')

    def merge_regions(self, outputs=None, tol: float = 1e-8, law_tol: float = 1e-8, device: int = 0) -> 'Solution':
        """A new solution whose regions are convex unions of this one's regions with the same law on the rows ``outputs`` of x (None:
        all rows); greedy pairwise merging in rounds on the device, deterministic and pairwise maximal (region_merge.py).
        Every region of the result is a region_merge.MergedRegion with the law x[outputs] = A theta + b and the ascending source indices
        ``members``.  ValueError before any launch for overlapping (mpLP) and mixed-integer sources, n_theta > 16, a region of more than
        256 rows and outputs out of range."""
        from .region_merge import merge_regions
        return merge_regions(self, outputs=outputs, tol=tol, law_tol=law_tol, device=device)

    def remove_overlaps(self, tol: float = 1e-8, value_tol: float = 1e-9, max_pieces: int = 1 << 20, device: int = 0,
                        reduce_rows: bool = False, sweep: str = 'host', screen: str = 'none') -> 'Solution':
        """A new, non-overlapping solution: every region keeps only the part of the parameter space where its value function is the
        lowest among the regions that contain the point (ties to the higher index, as get_region resolves them), as convex pieces
        (overlap.ReducedRegion with ``source``), ordered by source; the pair comparisons and the region differences are LPs on the device
        (overlap.py).  ``overlap_info`` of the result holds the source, sources, verdict_counts, vanished and stats.
        ValueError before any launch for an empty or merged solution, n_theta > 16, a region of more than 256 rows, non-finite
        tolerances and value functions with different quadratic parts (mpQP / mpMIQP); after a round for a piece of more than 256
        rows or more than max_pieces pieces.  ``reduce_rows``: the pieces lose their redundant rows round by round on the device, before
        the row limit is checked (off by default).  ``sweep`` = 'device' lists the candidate pairs on the device (the same
        list), ``screen`` = 'rows' drops the candidates one row already separates; the result is the same either way."""
        from .overlap import remove_overlaps
        return remove_overlaps(self, tol=tol, value_tol=value_tol, max_pieces=max_pieces, device=device, reduce_rows=reduce_rows, sweep=sweep,
                               screen=screen)

    def reduce_rows(self, tol: float = 1e-8, device: int = 0) -> 'Solution':
        """A new solution whose regions have lost their redundant rows by the sequential rule of geometry.reduce, for
        the results of merge_regions and remove_overlaps: every region is copied and only its E, f are replaced by the rows that are kept,
        in order and with their bits unchanged; merge_info and overlap_info are carried over and ``reduce_info`` holds the stats.  The
        source is not modified.  ValueError before any launch for other solutions, n_theta > 16, a region of more than 512 rows and a
        tol that is not finite and >= 0."""
        from .geometry.reduce import reduce_solution
        return reduce_solution(self, tol=tol, device=device)

    def output_range(self, outputs=None, tol: float = 1e-8, device: int = 0):
        """The bounds the explicit controller can command: a geometry.support.OutputRange with lo[i, k] and hi[i, k], the smallest and
        largest value of row outputs[k] of the law A_i theta + b_i over region i (None: every row the regions keep), arg_lo and arg_hi
        where they are attained, and flag for an entry that is a bound and not a value (an unbounded region, or the pivot cap); two LPs
        per region and row on the device, in the order row 0 max, row 0 min, row 1 max, ...; a constant row costs none and gives lo = hi
        = b_i[k] exactly.  ``overall()`` gives the extremes over all regions.  The regions are the rows the locator holds, scaled to unit
        normals.  ValueError before any launch for an empty solution, n_theta > 16, a region of more than 512 rows, a row a merged
        solution did not keep and a tol that is not finite and >= 0.  See DESIGN §3.28."""
        from .geometry.support import output_range
        return output_range(self, outputs=outputs, tol=tol, device=device)

    def compare(self, other: 'Solution', outputs=None, tol: float = 1e-8, ranges: bool = False, coverage: bool = False, device: int = 0,
                sweep: str = 'host', screen: str = 'none'):
        """How far this solution's law is from ``other``'s, exactly: a compare.LawGap.  For every region i of this solution and j of the
        other whose intersection has a Chebyshev radius above tol: the largest |x_self - x_other| over it in any of the rows ``outputs`` of
        the program's x (None: all rows), the lowest row that attains it and the theta where it does, by one radius LP and up to two LPs
        per row on the device; max_gap, worst, gap_of_a / gap_of_b, unmatched_a / unmatched_b and equal(atol) summarise them.  A merged
        solution is compared on the rows it kept.  ``ranges``: the minimum and maximum of every row's difference per pair; ``coverage``:
        the share of every region's volume that the other side's meeting regions cover.  ValueError before any launch for an empty
        solution, different n_theta, n_theta > 16, a region of more than 256 rows, a row the merged solution did not keep and a solution
        flagged overlapping (use remove_overlaps() first).  ``sweep`` = 'device' lists the candidate pairs on the device (the same list,
        the same result bit for bit); ``screen`` = 'rows' drops the candidates one row already separates, and the per-pair arrays then hold
        the kept candidates only.  See compare.py and DESIGN §3.26."""
        from .compare import compare_solutions
        return compare_solutions(self, other, outputs=outputs, tol=tol, ranges=ranges, coverage=coverage, device=device, sweep=sweep,
                                 screen=screen)

    def evaluate_objective(self, theta_point) -> Optional[float]:
        self._refuse_merged('evaluate_objective')
        x = self.evaluate(theta_point)
        return None if x is None else self.program.evaluate_objective(x, theta_point)

    # ---- batched point location on the device (the loop of get_region / evaluate over many parameter points) --------------
    def _stacked(self):
        """([f | E] rows of all regions, row offsets, [b | A] of all regions), in list order."""
        from .region_batch import BatchCriticalRegion
        regs = self.critical_regions
        n_t = self.program.num_t() if self.program is not None else regs[0].E.shape[1]
        ef_parts, cnt, xl_parts = [], [], []
        adj_masks, adj_info, adj_ok = [], [], True       # facet adjacency for the walk locator (device-solved regions only)
        n_c = self.program.num_constraints() if hasattr(self.program, 'num_constraints') else 0
        adj_ok = n_c > 0 and n_t > 1       # one parameter: regions are intervals built by the 1-D variant, whose two rows carry no facet kinds
        words = 2 if n_c <= 128 else 4
        i = 0
        while i < len(regs):
            r = regs[i]
            if isinstance(r, BatchCriticalRegion) and '_batch' in r.__dict__ and r.y_fixation is None:
                # a run of regions backed by the same level arrays: cut everything out with index arithmetic
                B = r._batch
                j = i
                while j < len(regs) and isinstance(regs[j], BatchCriticalRegion) and regs[j].__dict__.get('_batch') is B \
                        and regs[j].y_fixation is None:
                    j += 1
                slots = numpy.fromiter((q._j for q in regs[i:j]), dtype=numpy.int64, count=j - i)
                nE, off = B.hi[slots, 2].astype(numpy.int64), B.hi[slots, 6].astype(numpy.int64)
                rows = numpy.repeat(off - numpy.concatenate([[0], numpy.cumsum(nE)[:-1]]), nE) + numpy.arange(int(nE.sum()))
                ef_parts.append(B.er[rows])
                cnt.append(nE)
                A = B.hd[slots, B.oA:B.ob].reshape(len(slots), B.n_x, B.n_t)
                b = B.hd[slots, B.ob:B.oC].reshape(len(slots), B.n_x, 1)
                xl_parts.append(numpy.concatenate([b, A], axis=2))
                if adj_ok:
                    # rows of E in order: kept multiplier rows (lambda_set), kept inactive rows (regular_set[1]), kept A_t rows
                    # (omega_set); a region that lost exact duplicate rows (fewer rows than entries) gets kind "unknown"
                    hi = B.hi[slots]
                    la = hi[:, B.ila:B.ila + B.k]
                    rc_ = hi[:, B.irc:B.irc + (B.n_c - B.k)]
                    om = hi[:, B.iom:B.iom + B.n_tc]
                    pad = numpy.concatenate([numpy.where(la >= 0, la, -1), numpy.where(rc_ >= 0, rc_ + (1 << 16), -1),
                                             numpy.where(om >= 0, om + (2 << 16), -1)], axis=1)
                    n_lists = (pad >= 0).sum(axis=1)
                    good = n_lists == nE
                    info = pad[pad >= 0]
                    if not good.all():
                        # rebuild per region: unknown rows where the counts disagree
                        parts, pos = [], 0
                        for q in range(len(slots)):
                            seg = info[pos:pos + n_lists[q]]
                            pos += n_lists[q]
                            parts.append(seg if good[q] else numpy.full(int(nE[q]), 3 << 16, dtype=numpy.int64))
                        info = numpy.concatenate(parts) if parts else info
                    adj_info.append(info.astype(numpy.int32))
                    act = hi[:, B.iact:B.iact + B.k].astype(numpy.int64)
                    mk = numpy.zeros((len(slots), words), dtype=numpy.uint64)
                    for col in range(B.k):
                        numpy.bitwise_or.at(mk, (numpy.arange(len(slots)), act[:, col] >> 6),
                                            numpy.uint64(1) << (act[:, col] & 63).astype(numpy.uint64))
                    adj_masks.append(mk)
                i = j
            else:
                ef_parts.append(numpy.hstack([numpy.asarray(r.f, dtype=float).reshape(-1, 1), numpy.asarray(r.E, dtype=float).reshape(-1, n_t)]))
                cnt.append(numpy.array([ef_parts[-1].shape[0]], dtype=numpy.int64))
                bx, Ax = numpy.asarray(r.b, dtype=float).reshape(-1, 1), numpy.asarray(r.A, dtype=float).reshape(-1, n_t)
                if r.y_fixation is not None:
                    # region of a mixed-integer solution (whose E, f may have been replaced by the overlap reduction): the
                    # law of the full variable vector, binaries as constant rows (critical_region.py:64-77)
                    n_full = len(r.x_indices) + len(r.y_indices)
                    b_full, A_full = numpy.zeros((n_full, 1)), numpy.zeros((n_full, n_t))
                    b_full[r.x_indices], A_full[r.x_indices] = bx, Ax
                    b_full[r.y_indices, 0] = r.y_fixation
                    bx, Ax = b_full, A_full
                xl_parts.append(numpy.concatenate([bx[None], Ax[None]], axis=2))
                # a hand-built region carries its index sets too, but not necessarily in row order: no walk through it
                adj_info.append(numpy.full(ef_parts[-1].shape[0], 3 << 16, dtype=numpy.int32))
                mk = numpy.zeros((1, words), dtype=numpy.uint64)
                for v in (r.active_set if r.y_fixation is None else []):
                    mk[0, int(v) >> 6] |= numpy.uint64(1) << numpy.uint64(int(v) & 63)
                adj_masks.append(mk)
                if r.y_fixation is not None:
                    adj_ok = False        # regions of different fixations share active sets
                i += 1
        counts = numpy.concatenate(cnt) if cnt else numpy.zeros(0, dtype=numpy.int64)
        row_off = numpy.concatenate([[0], numpy.cumsum(counts)]).astype(numpy.int64)
        self._adjacency = (numpy.concatenate(adj_masks, axis=0), numpy.concatenate(adj_info)) if adj_ok and adj_masks else None
        return numpy.vstack(ef_parts), row_off, numpy.concatenate(xl_parts, axis=0)

    def locator(self, device: int = 0):
        """The device-resident copy of the regions; rebuilt when the region list has changed."""
        from . import _lib
        key = (len(self.critical_regions), id(self.critical_regions[0]) if self.critical_regions else 0,
               id(self.critical_regions[-1]) if self.critical_regions else 0, device)
        if getattr(self, '_locator_key', None) != key:
            if getattr(self, '_locator', None) is not None:
                self._locator.close()
            ef, row_off, xlaw = self._stacked()
            P = self.program
            # a merged solution's laws hold only the rows of x it was merged for, and it is never overlapping: no objective, no walk
            P_obj = None if self.merge_info is not None else P
            self._locator = _lib.Locator(row_off, ef, xlaw, getattr(P_obj, 'Q', None), getattr(P_obj, 'c', None), getattr(P_obj, 'H', None), device)
            adj = getattr(self, '_adjacency', None)
            # (nor through a reduced one: the pieces of one source share its active set)
            if adj is not None and self.merge_info is None and self.overlap_info is None and len(adj[1]) == int(row_off[-1]) and len(self.critical_regions) >= self.WALK_MIN_REGIONS:
                self._locator.set_adjacency(adj[0], adj[1], P.num_constraints())
            self._locator_key = key
        return self._locator

    def get_region_batch(self, theta_points: numpy.ndarray, device: int = 0, inclusive: bool = False) -> numpy.ndarray:
        """Index into critical_regions of get_region(theta) for every row of theta_points (-1: no region)
        (solution.py:60-112, all points at once on the GPU).  ``inclusive``: membership is ``E theta <= f + tol`` instead
        of get_region's strict ``E theta - f < tol`` (used by upop.PointLocation with tol = 0)."""
        if not self.critical_regions:
            return numpy.full(len(numpy.atleast_2d(theta_points)), -1, dtype=numpy.int64)
        return self.locator(device).query(theta_points, self.point_location_tolerance, self.is_overlapping, want_x=False,
                                          inclusive=inclusive, walk=self.use_walk and self.is_complete)[0]

    def evaluate_batch(self, theta_points: numpy.ndarray, device: int = 0, inclusive: bool = False):
        """(x* [m, n_x] (NaN rows where no region contains the point), region index [m])  -- evaluate() for many points."""
        th = numpy.atleast_2d(numpy.asarray(theta_points, dtype=float))
        if not self.critical_regions:
            return numpy.full((len(th), 0), numpy.nan), numpy.full(len(th), -1, dtype=numpy.int64)
        region, x = self.locator(device).query(th, self.point_location_tolerance, self.is_overlapping, want_x=True,
                                               inclusive=inclusive, walk=self.use_walk and self.is_complete)
        return x, region

    def search_tree(self, **kw):
        """A point-location search tree of this solution (upop.SearchTree.build(self, **kw)), built once per locator and
        keyword set; get_region_batch / evaluate_batch keep scanning -- use the tree's locate_batch / evaluate_batch."""
        from .upop.search_tree import SearchTree
        device = int(kw.get('device', 0))
        self.locator(device)
        key = (self._locator_key, tuple(sorted(kw.items())))
        cache = getattr(self, '_search_trees', None)
        if cache is None or cache[0] != self._locator_key:
            cache = (self._locator_key, {})
            self._search_trees = cache
        if key not in cache[1]:
            cache[1][key] = SearchTree.build(self, **kw)
        return cache[1][key]

    def vertices(self, tol: float = 1e-9, device: int = 0):
        """The V-representation of every region (geometry.vertices.RegionVertices: vertices, offsets, incidence, rays, status, stats),
        enumerated on the device from the rows the locator holds; built once per locator and tol.  See DESIGN §3.16."""
        from .geometry.vertices import vertices_of_rows
        self.locator(device)
        cache = getattr(self, '_vertex_sets', None)
        if cache is None or cache[0] != self._locator_key:
            cache = (self._locator_key, {})
            self._vertex_sets = cache
        if tol not in cache[1]:
            ef, row_off, _ = self._stacked()
            n_t = ef.shape[1] - 1
            cache[1][tol] = vertices_of_rows(row_off, ef, n_t, tol=tol, device=device, who='Solution.vertices')
        return cache[1][tol]

    def volumes(self, tol: float = 1e-9, max_simplices=None, device: int = 0):
        """The volume and centroid of every region (geometry.volume.RegionVolumes: volume, centroid, simplices, status, stats, vertices),
        triangulated on the device from the vertex lists of ``vertices(tol)``; one entry per region.  See DESIGN §3.17."""
        from .geometry.volume import volumes_of_rows
        rv = self.vertices(tol=tol, device=device)
        ef, row_off, _ = self._stacked()
        return volumes_of_rows(row_off, ef, ef.shape[1] - 1, tol=tol, max_simplices=max_simplices, device=device, who='Solution.volumes', vertices=rv)

    def moments(self, tol: float = 1e-9, max_simplices=None, device: int = 0):
        """Volume, centroid and second moment (the integral of theta theta^T) of every region: a geometry.moments.RegionMoments, from the
        vertex lists of ``vertices(tol)`` like ``volumes()``, whose volume, centroid, simplices and status it repeats bit for bit.  See
        DESIGN §3.18."""
        from .geometry.moments import moments_of_rows
        rv = self.vertices(tol=tol, device=device)
        ef, row_off, _ = self._stacked()
        return moments_of_rows(row_off, ef, ef.shape[1] - 1, tol=tol, max_simplices=max_simplices, device=device, who='Solution.moments', vertices=rv)

    def value_function(self):
        """(Qv [R, n, n], qv [R, n], rv [R]): J*(theta) = 1/2 theta^T Qv theta + qv^T theta + rv on region R, the objective of
        ``program.evaluate_objective`` along the region's law x = A theta + b.  ValueError for a merged solution."""
        from .geometry.moments import value_function
        return value_function(self)

    def expected_values(self, max_simplices=None, device: int = 0):
        """Exact averages for theta uniform on the union of the OK regions: a geometry.moments.ExpectedValues with the volume, the
        integral and the mean of the value function, mean and covariance of x* and of theta, the integral and volume per region,
        status_counts and ok (no region left undecided).  ValueError for overlapping (mpLP), mixed-integer and merged solutions.  See
        DESIGN §3.18."""
        from .geometry.moments import expected_values
        return expected_values(self, max_simplices=max_simplices, device=device)

    def coverage_volume(self, device: int = 0):
        """The exact share of the parameter space {A_t theta <= b_t} the regions cover: a geometry.volume.CoverageVolume with total (the
        summed volume of the OK regions), theta_volume, fraction, status_counts and ok (no region left undecided).  ValueError for
        overlapping (mpLP) and mixed-integer solutions, whose regions may overlap; merged solutions and the results of remove_overlaps
        are fine.  See DESIGN §3.17."""
        from .geometry.volume import coverage_volume
        return coverage_volume(self, device=device)

    def certify_recursive_feasibility(self, A, B, inputs, c=None, disturbance=None, tol: float = 1e-7, device: int = 0):
        """Whether the plant theta+ = A theta + B u + c (+ a box disturbance (lo, hi)) under this controller's law u = x*(theta)[inputs]
        stays where the program is feasible, region by region: an invariance.FeasibilityCertificate.  See
        invariance.certify_recursive_feasibility and DESIGN §3.16."""
        from .invariance import certify_recursive_feasibility
        return certify_recursive_feasibility(self, A, B, inputs, c=c, disturbance=disturbance, tol=tol, device=device)

    def transition_graph(self, A, B, inputs, c=None, tol: float = 1e-8, full_radius: bool = False, device: int = 0, sweep: str = 'host',
                         screen: str = 'none'):
        """Which region can follow which under the plant theta+ = A theta + B u + c with this controller's law u = x*(theta)[inputs]: a
        transition.TransitionGraph (successors in CSR form, per edge radius, status and witness; reachable, steps_to, cycles_outside).
        i -> j is an edge iff {theta in R_i : its image lies in R_j} has a Chebyshev radius above tol, one LP per candidate pair on the
        device; ``full_radius`` runs every LP to its optimum.  Transitions through a facet or a vertex are not edges, so statements about
        trajectories hold for almost every initial state.  ValueError before any launch for mixed-integer solutions, solutions flagged
        overlapping that have not been through remove_overlaps, and the arguments certify_recursive_feasibility refuses; merged
        solutions and reduced continuous ones are accepted.  ``sweep`` = 'device' lists the candidate pairs on the device (the same list),
        ``screen`` = 'rows' drops the candidates that a row of the target separates from the image box; the graph is the same
        either way.  See transition.py and DESIGN §3.20."""
        from .transition import transition_graph
        return transition_graph(self, A, B, inputs, c=c, tol=tol, full_radius=full_radius, device=device, sweep=sweep, screen=screen)

    def exit_sets(self, A, B, inputs, c=None, tol: float = 1e-8, graph=None, max_pieces: int = 1 << 20, device: int = 0,
                  reduce_rows: bool = False):
        """Where each region's next state leaves the solution under the plant theta+ = A theta + B u + c with this controller's law
        u = x*(theta)[inputs]: an exit_sets.ExitSets, the convex pieces of Chebyshev radius above tol of X_i = R_i minus the states whose
        image lies in some region (pieces_of, contains, polytopes, volumes; whole[i]: region i leaves entirely).  The regions cut out of
        R_i are its successors in ``graph``, the transition_graph of the same arguments (built when None); one device launch per round
        of the region difference.  A run that is unbounded or capped keeps its piece and flags it wide: the pieces never lose a state
        that exits.  Refusals as for transition_graph, and ValueError after a round that leaves a piece above 256 rows or more than
        max_pieces pieces.  ``reduce_rows``: the pieces lose their redundant rows round by round on the device, before the row limit is
        checked (off by default); ExitSets.reduced() does the same to a finished result.  A graph built with
        transition_graph(sweep='device', screen='rows') is passed as ``graph``; no argument of its own is needed.  See exit_sets.py and
        DESIGN §3.21."""
        from .exit_sets import exit_sets
        return exit_sets(self, A, B, inputs, c=c, tol=tol, graph=graph, max_pieces=max_pieces, device=device, reduce_rows=reduce_rows)

    def invariant_set(self, A, B, inputs, c=None, tol: float = 1e-8, graph=None, exits=None, max_steps: int = 64, max_cells: int = 1 << 20,
                      reduce_rows: bool = True, device: int = 0):
        """From which states the loop under the plant theta+ = A theta + B u + c with this controller's law u = x*(theta)[inputs] stays
        inside the solution for ever, and after how many steps the others leave: an invariant_set.InvariantSet, the cells of radius above
        tol whose states leave after exactly step + 1 steps (cells_of, exit_step, contains, polytopes, volumes, pieces).  Step 0 is
        ``exits``, the exit_sets of the same arguments, the predecessors come from ``graph``, the transition_graph (each built when None);
        every later step runs on the device inside one library call, until a step yields no cell (converged) or max_steps, max_cells or
        the 256-row limit of a cell stops it (status).  Wide cells over-approximate what leaves; parts thinner than tol are not reported.
        Refusals as for transition_graph.  A graph built with transition_graph(sweep='device', screen='rows') is passed as ``graph``.
        See invariant_set.py and DESIGN §3.23."""
        from .invariant_set import invariant_set
        return invariant_set(self, A, B, inputs, c=c, tol=tol, graph=graph, exits=exits, max_steps=max_steps, max_cells=max_cells,
                             reduce_rows=reduce_rows, device=device)

    def reach_cells(self, A, B, inputs, c=None, initial=None, steps: int = 8, tol: float = 1e-8, graph=None, max_cells: int = 1 << 20,
                    max_rows_total=None, device: int = 0):
        """Where the states of ``initial`` (a Polytope, a list of them, or None: the regions themselves) are after 1 .. ``steps`` steps of
        the loop under the plant theta+ = A theta + B u + c with this controller's law u = x*(theta)[inputs]: a reach.ForwardCells, cells
        of INITIAL states of radius above tol, each with the region it is in at its step, the composed map theta_k = G theta_0 + g and
        its parent (cells_at, itinerary, locate, state_at, volumes, image_vertices, images, entering: the safety and target query).
        The successors come from ``graph``, the transition_graph of the same arguments (built when None); every step runs on the
        device inside one library call.  No map is inverted: singular and contracting loops are followed like any other.  Refusals as
        for transition_graph.  A graph built with transition_graph(sweep='device', screen='rows') is passed as ``graph``.  See reach.py
        and DESIGN §3.25."""
        from .reach import reach_cells
        return reach_cells(self, A, B, inputs, c=c, initial=initial, steps=steps, tol=tol, graph=graph, max_cells=max_cells,
                           max_rows_total=max_rows_total, device=device)

    def simulate(self, theta0, steps: int, A, B, inputs, c=None, disturbance=None, seed: int = 0, stop_tol=None, locate: str = 'auto',
                 record: str = 'full', inclusive: bool = False, device: int = 0):
        """This explicit controller in closed loop with the plant theta+ = A theta + B u + c + w, u = x*(theta)[inputs], for many initial
        states in one device launch: a closed_loop.ClosedLoopResult (theta, u, region, status, exit_step, stats).  See
        closed_loop.simulate and DESIGN §3.15."""
        from .closed_loop import simulate
        return simulate(self, theta0, steps, A, B, inputs, c=c, disturbance=disturbance, seed=seed, stop_tol=stop_tol, locate=locate,
                        record=record, inclusive=inclusive, device=device)

    # ---- verification without a QP solver: the KKT conditions of the program at theta ----------------------------------------
    def kkt_residuals(self, region: CriticalRegion, theta_point: numpy.ndarray) -> dict:
        """Largest violation of each optimality condition of the program at ``theta_point`` by the region's laws
        x* = A theta + b, lambda* = C theta + d: primal feasibility, multiplier sign, stationarity, complementarity
        (all scaled by 1 + the magnitude of the quantities involved)."""
        self._refuse_merged('kkt_residuals')
        P = self.program
        th = numpy.asarray(theta_point, dtype=float).reshape(-1, 1)
        x = numpy.asarray(region.A) @ th + numpy.asarray(region.b).reshape(-1, 1)
        lam = numpy.asarray(region.C) @ th + numpy.asarray(region.d).reshape(-1, 1)
        aset = list(region.active_set)
        n_eq = len(P.equality_indices)
        rhs = P.b + P.F @ th
        slack = rhs - P.A @ x
        scale = 1.0 + numpy.abs(rhs)
        primal = float(numpy.max(numpy.concatenate([(-slack / scale)[n_eq:].ravel(), (numpy.abs(slack) / scale)[:n_eq].ravel(), [0.0]])))
        grad = P.H @ th + P.c + P.A[aset].T @ lam
        if hasattr(P, 'Q'):
            grad = grad + P.Q @ x
        stationarity = float(numpy.max(numpy.abs(grad)) / (1.0 + numpy.max(numpy.abs(P.c)) + numpy.max(numpy.abs(lam), initial=0.0)))
        ineq = [j for j, i in enumerate(aset) if i >= n_eq]
        sign = float(max(0.0, -numpy.min(lam[ineq], initial=0.0)) / (1.0 + numpy.max(numpy.abs(lam), initial=0.0)))
        compl = float(numpy.max(numpy.abs(slack[aset]) / scale[aset], initial=0.0))
        return {'primal': primal, 'multiplier_sign': sign, 'stationarity': stationarity, 'complementarity': compl}

    def verify_theta(self, theta_point: numpy.ndarray, tol: float = 1e-6) -> bool:
        """Is the explicit solution optimal for the program at ``theta_point``?  The reference compares with a
        deterministic solve (solution.py:149-174); here the region's own x*(theta), lambda*(theta) are put through the
        KKT conditions, which are sufficient for the convex programs of this package and need no QP solver.  A point
        in no region verifies when the program is infeasible there (one LP on the device)."""
        self._refuse_merged('verify_theta')
        region = self.get_region(theta_point)
        P = self.program
        th = numpy.asarray(theta_point, dtype=float).reshape(-1, 1)
        if self.is_mixed_integer_sol():
            # the reference's rule by objective (solution.py:149-174): no region exactly where the deterministic solve has no
            # solution, else the region's objective is the optimum
            if region is None:
                return True if not P.valid_parameter_realization(th) else P.solve_theta(th) is None
            det = P.solve_theta(th)
            if det is None:
                return False
            here = P.evaluate_objective(region.evaluate(th), th)
            return abs(here - det.obj) <= tol * (1.0 + abs(det.obj))
        if region is None:
            if not P.valid_parameter_realization(th):
                return True
            feasible = P.solver.solve_lp(None, P.A, P.b + P.F @ th, P.equality_indices) is not None
            return not feasible
        return max(self.kkt_residuals(region, theta_point).values()) <= tol

    def chebyshev_centres(self, device: int = 0):
        """(centres [R, n_theta], radii [R]) of all regions: the Chebyshev LPs of every region (chebyshev_ball.py:10-63)
        as ONE batch on the device, rows padded to the largest region."""
        from . import _lib
        regs = self.critical_regions
        n_t = self.program.num_t()
        rows = max(numpy.asarray(r.E).shape[0] for r in regs) + 1
        A = numpy.zeros((len(regs), rows, n_t + 1))
        b = numpy.ones((len(regs), rows))
        for i, r in enumerate(regs):
            E = numpy.asarray(r.E, dtype=float).reshape(-1, n_t)
            m = E.shape[0]
            A[i, :m, :n_t] = E
            A[i, :m, n_t] = numpy.linalg.norm(E, axis=1)
            b[i, :m] = numpy.asarray(r.f, dtype=float).reshape(-1)
            A[i, m, n_t] = -1.0            # -r <= 0
            b[i, m] = 0.0
        c = numpy.zeros(n_t + 1)
        c[n_t] = -1.0
        status, x, _, _ = _lib.lp_solve_batch(A, b, c, numpy.zeros((len(regs), rows), dtype=numpy.uint8), device=device)
        radii = numpy.where(status == _lib.LP_OPTIMAL, x[:, n_t], numpy.nan)
        return x[:, :n_t], radii

    def verify_solution(self, tol: float = 1e-6, device: int = 0) -> bool:
        """Every region is optimal at its own Chebyshev centre and, without overlaps, is the region found there
        (solution.py:114-147 with the KKT conditions in place of the deterministic solve)."""
        self._refuse_merged('verify_solution')
        if not self.critical_regions:
            return True
        centres, radii = self.chebyshev_centres(device)
        if numpy.any(~numpy.isfinite(radii)):
            return False
        located = self.get_region_batch(centres, device)
        if self.is_mixed_integer_sol():
            return self._verify_mixed_integer(centres, located, tol)
        # the reference's own test where the program offers it: the deterministic solve at the centre (one device batch of QPs
        # / LPs, MPQP_Program.solve_theta_batch) must give the region's x* -- solution.py:128-145
        det = None
        if hasattr(self.program, 'solve_theta_batch') and all(r.y_fixation is None for r in self.critical_regions):
            try:
                det = self.program.solve_theta_batch(centres)
            except Exception:          # e.g. a positive semidefinite Q: the QP batch does not apply, the KKT test below stands alone
                det = None
        for i, region in enumerate(self.critical_regions):
            if max(self.kkt_residuals(region, centres[i]).values()) > tol:
                return False
            if det is not None and det[i] is not None and not self.is_overlapping:
                xr = region.evaluate(centres[i].reshape(-1, 1)).ravel()
                if numpy.max(numpy.abs(det[i].sol - xr)) > 1e-5 * (1.0 + numpy.max(numpy.abs(xr))):
                    return False
            if not self.is_overlapping and located[i] != i:
                # a thin region (radius below the point-location tolerance) may be preceded in the list by a neighbour that
                # contains the centre within that tolerance: consistent as long as both give the same objective there
                if located[i] < 0:
                    return False
                th = centres[i].reshape(-1, 1)
                here = self.program.evaluate_objective(region.evaluate(th), th)
                there = self.program.evaluate_objective(self.critical_regions[int(located[i])].evaluate(th), th)
                if abs(here - there) > tol * (1.0 + abs(here)):
                    return False
        return True

    def _verify_mixed_integer(self, centres: numpy.ndarray, located: numpy.ndarray, tol: float) -> bool:
        """verify_solution of a mixed-integer solution, by objective: the deterministic optimum at every Chebyshev centre (one
        solve_theta_batch) is the objective of the region located there, and no region's own objective lies below it."""
        P = self.program
        det = P.solve_theta_batch(centres)
        for i, region in enumerate(self.critical_regions):
            if det[i] is None or located[i] < 0:
                return False
            th = centres[i].reshape(-1, 1)
            opt = det[i].obj
            there = P.evaluate_objective(self.critical_regions[int(located[i])].evaluate(th), th)
            own = P.evaluate_objective(region.evaluate(th), th)
            if abs(there - opt) > tol * (1.0 + abs(opt)) or own < opt - tol * (1.0 + abs(opt)):
                return False
        return True

    # ---- coverage and optimality away from the centres: uniform samples of the parameter set and of every region ------------
    def _objective_rows(self, X: numpy.ndarray, T: numpy.ndarray) -> numpy.ndarray:
        """program.evaluate_objective for every row of X [m, n_x] at T [m, n_theta]."""
        P = self.program
        v = X @ numpy.asarray(P.c, dtype=float).ravel() + numpy.einsum('ij,ij->i', T @ numpy.asarray(P.H, dtype=float).T, X)
        v = v + float(numpy.asarray(P.c_c).ravel()[0]) + T @ numpy.asarray(P.c_t, dtype=float).ravel()
        v = v + 0.5 * numpy.einsum('ij,ij->i', T @ numpy.asarray(P.Q_t, dtype=float), T)
        if hasattr(P, 'Q'):
            v = v + 0.5 * numpy.einsum('ij,ij->i', X @ numpy.asarray(P.Q, dtype=float), X)
        return v

    def _row_violation(self, X: numpy.ndarray, T: numpy.ndarray) -> numpy.ndarray:
        """Largest violation of a program row A x <= b + F theta (equalities in both directions) by every row of X."""
        P = self.program
        r = X @ P.A.T - (P.b.reshape(1, -1) + T @ P.F.T)
        eq = list(P.equality_indices)
        if eq:
            r[:, eq] = numpy.abs(r[:, eq])
        return numpy.max(r, axis=1, initial=0.0)

    def sample_check(self, num_samples: int = 100_000, per_region: int = 8, seed: int = 0, tol: float = 1e-6, device: int = 0,
                     n_steps: Optional[int] = None) -> SampleCheck:
        """Does the solution cover the feasible parameter set, and is every region's law optimal away from its centre?
        Global part: ``num_samples`` points drawn uniformly from {A_t theta <= b_t} (geometry.sample_program_theta_space), the
        program solved at all of them (one solve_theta_batch) and the points located (one get_region_batch); a feasible point in
        no region is uncovered, a located point whose law is worse than the optimum (objective gap above tol (1 + |obj*|) or a row
        violated by more than tol) is wrong.  Per-region part: ``per_region`` hit-and-run samples in every full-dimensional region
        (one mpc_hit_and_run over all regions, from the Chebyshev centres), the same test on the region's own law; for
        mixed-integer solutions the rule of _verify_mixed_integer (own objective not below the optimum, located winner equal to it).
        MpcError for an unbounded parameter set and wherever solve_theta_batch raises."""
        self._refuse_merged('sample_check')
        from . import _lib
        from .geometry import polytope_operations as po
        t0 = time.perf_counter()
        P = self.program
        steps = po.DEFAULT_N_STEPS if n_steps is None else int(n_steps)
        mi = self.is_mixed_integer_sol()
        is_qp = hasattr(P, 'Q') and not mi
        scale = lambda o: tol * (1.0 + numpy.abs(o))

        # global part: coverage of the parameter set
        th = po.sample_program_theta_space(P, num_samples, n_steps=steps, seed=seed, device=device)
        det = P.solve_theta_batch(th)
        feas = numpy.array([d is not None for d in det], dtype=bool)
        if self.critical_regions:
            x_r, loc = self.evaluate_batch(th, device)
        else:
            x_r, loc = numpy.full((len(th), 0), numpy.nan), numpy.full(len(th), -1, dtype=numpy.int64)
        located = loc >= 0
        uncovered = feas & ~located
        max_gap, max_x, n_wrong, n_spur_bad = 0.0, (0.0 if is_qp else None), 0, 0
        idx = numpy.flatnonzero(located & feas)
        if len(idx):
            opt = numpy.array([det[i].obj for i in idx])
            obj_r = self._objective_rows(x_r[idx], th[idx])
            viol = self._row_violation(x_r[idx], th[idx])
            gap = numpy.abs(obj_r - opt)
            max_gap = float(numpy.max(gap / (1.0 + numpy.abs(opt))))
            n_wrong = int(numpy.count_nonzero((gap > scale(opt)) | (viol > tol)))
            if is_qp:
                max_x = float(numpy.max(numpy.abs(x_r[idx] - numpy.vstack([det[i].sol.ravel() for i in idx]))))
        spur = numpy.flatnonzero(located & ~feas)
        if len(spur):
            n_spur_bad = int(numpy.count_nonzero(self._row_violation(x_r[spur], th[spur]) > tol))

        # per-region part: each region's own law at uniform points inside it
        failing, n_sampled, n_not = set(), 0, len(self.critical_regions)
        if self.critical_regions and per_region > 0:
            loc_obj = self.locator(device)
            row_off, ef, xlaw = loc_obj.row_off, loc_obj.ef, loc_obj.xlaw
            centres, radii = self.chebyshev_centres(device)
            counts = numpy.diff(row_off)
            ok_r = numpy.flatnonzero(numpy.isfinite(radii) & (radii > po.FULL_DIM_RADIUS) & (counts <= _lib.HR_MAX_ROWS) & (counts > 0))
            if len(ok_r):
                sub_off = numpy.concatenate([[0], numpy.cumsum(counts[ok_r])]).astype(numpy.int64)
                sub_rows = numpy.repeat(row_off[ok_r] - sub_off[:-1], counts[ok_r]) + numpy.arange(int(sub_off[-1]))
                pts, status = _lib.hit_and_run(sub_off, ef[sub_rows], centres[ok_r], per_region, 1, steps, seed, device)
                good = status == _lib.MPC_HR_OK                                   # [R_s, per_region]
                n_sampled = int(numpy.count_nonzero(good.all(axis=1)))
                owner = numpy.repeat(ok_r, per_region)[good.ravel()]
                T = pts[:, :, 0, :].reshape(-1, pts.shape[-1])[good.ravel()]
                det_r = P.solve_theta_batch(T)
                feas_r = numpy.array([d is not None for d in det_r], dtype=bool)
                for r in owner[~feas_r]:
                    failing.add(int(r))          # a region's interior lies in the feasible set
                fi = numpy.flatnonzero(feas_r)
                if len(fi):
                    opt = numpy.array([det_r[i].obj for i in fi])
                    Tf = T[fi]
                    own_law = xlaw[owner[fi]]                                    # [k, n_x, n_t + 1]
                    X_own = own_law[:, :, 0] + numpy.einsum('kij,kj->ki', own_law[:, :, 1:], Tf)
                    own = self._objective_rows(X_own, Tf)
                    if mi:
                        x_w, loc_w = self.evaluate_batch(Tf, device)
                        there = numpy.where(loc_w >= 0, self._objective_rows(numpy.nan_to_num(x_w), Tf), numpy.nan)
                        bad = (own < opt - scale(opt)) | (loc_w < 0) | ~(numpy.abs(there - opt) <= scale(opt))
                    else:
                        bad = (numpy.abs(own - opt) > scale(opt)) | (self._row_violation(X_own, Tf) > tol)
                    failing.update(int(r) for r in owner[fi][bad])
            n_not = len(self.critical_regions) - n_sampled
        n_feas = int(numpy.count_nonzero(feas))
        return SampleCheck(n_samples=len(th), n_feasible=n_feas, n_uncovered=int(numpy.count_nonzero(uncovered)), n_wrong=n_wrong,
                           n_spurious=len(spur), n_spurious_bad=n_spur_bad,
                           covered_fraction=float(numpy.count_nonzero(located & feas) / n_feas) if n_feas else 1.0,
                           max_obj_gap=max_gap, max_x_err=max_x, uncovered_points=th[uncovered][:1000].copy(),
                           n_regions_sampled=n_sampled, n_regions_not_sampled=n_not, failing_regions=sorted(failing),
                           seconds=time.perf_counter() - t0)

    # ---- slices: the polygon of every region in a plane of parameter space, the interval on a line ----------------------------
    def _plane(self, dims, fixed, plane):
        """(theta_0 [n_t], U [n_t, 2], dims or None) of slice_2d's arguments; ValueError for arguments that do not fit."""
        n_t = self.theta_dim()
        if plane is not None:
            theta_0 = numpy.asarray(plane[0], dtype=float).reshape(-1)
            U = numpy.asarray(plane[1], dtype=float)
            if theta_0.shape != (n_t,) or U.shape != (n_t, 2):
                raise ValueError(f'plane must be (theta_0 [{n_t}], U [{n_t}, 2]), got {theta_0.shape} and {U.shape}')
            if numpy.linalg.matrix_rank(U) < 2:
                raise ValueError('the columns of U must be linearly independent')
            return theta_0, U, None
        dims = tuple(int(d) for d in dims)
        if len(dims) != 2 or dims[0] == dims[1] or not all(0 <= d < n_t for d in dims):
            raise ValueError(f'dims must be two different parameter indices in 0..{n_t - 1}, got {dims}')
        theta_0 = numpy.zeros(n_t)
        others = [t for t in range(n_t) if t not in dims]
        if isinstance(fixed, dict):
            if sorted(int(k) for k in fixed) != others:
                raise ValueError(f'fixed must give the parameters {others} (the ones not in dims), got {sorted(fixed)}')
            for k, v in fixed.items():
                theta_0[int(k)] = float(v)
        elif fixed is not None:
            f = numpy.asarray(fixed, dtype=float).reshape(-1)
            if f.shape != (n_t,):
                raise ValueError(f'fixed must be a full parameter vector of length {n_t} or a dict {{index: value}}, got length {f.size}')
            theta_0[others] = f[others]
        elif others:
            raise ValueError(f'the solution has {n_t} parameters: give fixed (values of {others}) or plane=(theta_0, U)')
        U = numpy.zeros((n_t, 2))
        U[dims[0], 0] = U[dims[1], 1] = 1.0
        return theta_0, U, dims

    def _plane_box(self, theta_0, U, device):
        """Bounding box (lo0, lo1, hi0, hi1) of {z : A_t (theta_0 + U z) <= b_t}: four LPs in one device batch."""
        from . import _lib
        P = self.program
        A = numpy.asarray(P.A_t, dtype=float) @ U
        b = numpy.asarray(P.b_t, dtype=float).reshape(-1) - numpy.asarray(P.A_t, dtype=float) @ theta_0
        k = U.shape[1]
        # bounded iff the normals of the reduced rows leave no open half-plane (half-line) free: checked here, before any launch
        nz = A[numpy.linalg.norm(A, axis=1) > 1e-12 * numpy.max(numpy.abs(A), initial=1e-300) * numpy.sqrt(k)]
        if k == 1:
            bounded = numpy.any(nz > 0) and numpy.any(nz < 0)
        else:
            ang = numpy.sort(numpy.arctan2(nz[:, 1], nz[:, 0]))
            bounded = len(ang) > 2 and numpy.max(numpy.diff(numpy.concatenate([ang, [ang[0] + 2 * numpy.pi]]))) < numpy.pi
        if not bounded:
            raise ValueError('the slice of the parameter set A_t theta <= b_t is unbounded; give box')
        c = numpy.vstack([numpy.eye(k), -numpy.eye(k)])
        status, x, obj, _ = _lib.lp_solve_batch(A, b, c, numpy.zeros((2 * k, len(b)), dtype=numpy.uint8), device=device)
        if numpy.any(status == _lib.LP_INFEASIBLE):
            raise ValueError('the slice misses the parameter set A_t theta <= b_t; give box')
        if numpy.any(status != _lib.LP_OPTIMAL):
            raise ValueError('the slice of the parameter set A_t theta <= b_t is unbounded; give box')
        return numpy.concatenate([obj[:k], -obj[k:]])

    def slice_2d(self, dims=(0, 1), fixed=None, plane=None, box=None, eps: Optional[float] = None, device: int = 0):
        """The polygon of every region in a plane of parameter space (geometry.SolutionSlice; one k_slice_polygons launch).
        The plane holds the parameters ``dims`` free and the others at ``fixed`` (a full parameter vector, or {index: value}); for two
        parameters nothing needs to be given.  ``plane=(theta_0, U)`` gives any plane theta = theta_0 + U z instead.  ``box`` =
        (lo0, lo1, hi0, hi1) bounds z; by default the bounding box of the parameter set's slice (four LPs), and ValueError when that is
        unbounded.  ``eps`` is the kernel's one tolerance (_lib.SLICE_EPS)."""
        from . import _lib
        from .geometry.slice import slice_rows
        theta_0, U, dims = self._plane(dims, fixed, plane)
        box = self._plane_box(theta_0, U, device) if box is None else numpy.asarray(box, dtype=float).reshape(-1)
        if box.shape != (4,) or not numpy.all(numpy.isfinite(box)) or not (box[0] < box[2] and box[1] < box[3]):
            raise ValueError(f'box must be (lo0, lo1, hi0, hi1), finite, with lo < hi; got {box}')
        ef, row_off, _ = self._stacked()
        return slice_rows(row_off, ef, theta_0, U, box, eps=_lib.SLICE_EPS if eps is None else eps, device=device, dims=dims)

    def slice_1d(self, theta_0, direction, t_range=None, eps: Optional[float] = None, device: int = 0):
        """The interval of every region on the line theta = theta_0 + direction t (geometry.LineSlice; one k_slice_intervals launch),
        with the laws' values x*(theta) at both ends.  ``t_range`` = (t_lo, t_hi) defaults to the line's extent in the parameter set
        (two LPs); ValueError when that is unbounded."""
        from . import _lib
        from .geometry.slice import LineSlice
        n_t = self.theta_dim()
        th0 = numpy.asarray(theta_0, dtype=float).reshape(-1)
        u = numpy.asarray(direction, dtype=float).reshape(-1)
        if th0.shape != (n_t,) or u.shape != (n_t,) or not numpy.any(u):
            raise ValueError(f'theta_0 and direction must be vectors of length {n_t}, direction nonzero')
        if t_range is None:
            lo, hi = self._plane_box(th0, u.reshape(-1, 1), device)
            t_range = (float(lo), float(hi))
        t_range = tuple(float(v) for v in t_range)
        if len(t_range) != 2 or not (numpy.isfinite(t_range).all() and t_range[0] < t_range[1]):
            raise ValueError(f't_range must be finite with t_lo < t_hi, got {t_range}')
        ef, row_off, xlaw = self._stacked()
        iv, st = _lib.slice_intervals(row_off, ef, th0, u, t_range, _lib.SLICE_EPS if eps is None else eps, device)
        ends = [th0 + iv[:, k:k + 1] * u for k in (0, 1)]        # [R, n_t], NaN rows for empty slices
        x = [xlaw[:, :, 0] + numpy.einsum('rij,rj->ri', xlaw[:, :, 1:], e) for e in ends]
        return LineSlice(regions=numpy.arange(len(st)), intervals=iv, status=st, theta_0=th0, direction=u, t_range=t_range,
                         x_start=x[0], x_end=x[1])

    def materialize(self) -> 'Solution':
        """Cuts every field of every region out of the per-level arrays the device returned (the regions a solve hands back are lazy
        views, ppopt_amd/region_batch.py) -- batch-wise, a few array operations per level.  Returns self."""
        from .region_batch import materialize_regions
        materialize_regions(self.critical_regions)
        return self

    def is_mixed_integer_sol(self) -> bool:
        from .mpmilp_program import MPMILP_Program
        return isinstance(self.program, MPMILP_Program)

    def theta_dim(self) -> int:
        return self.program.num_t()

    def __len__(self):
        return len(self.critical_regions)
