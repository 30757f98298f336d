"""Point-location search trees over an explicit solution's hyperplanes (Tøndel, Johansen & Bemporad, 2003).

A ``SearchTree`` is a binary tree over the unit planes s(theta) = n.theta - o of ``linear_code_gen.plane_table`` (the plane table
of the exported code).  It never changes an answer: for every point and every query tolerance up to the build tolerance, the
descent returns exactly the region the list scan returns (``Solution.get_region_batch``), in the strict and the inclusive mode,
also for overlapping solutions.  Region j is classified through its expanded polytope {E_i theta <= f_i + tol max(1, |E_i|)}
against every plane with a band w; a node keeps tau-/tau+ so that a query visits every child that may hold a region containing it.

The tree is built on the device (``mpc_tree_build``: k_tree_classify, k_tree_split, csrc/tree.hpp) and located on the device
(``locate_batch`` / ``evaluate_batch``: k_locate_tree) or on the host (``locate``, numpy, no device needed).
"""
from typing import Optional

import numpy

from .linear_code_gen import plane_table

__all__ = ['SearchTree']

_ARRAYS = ('planes', 'node_plane', 'node_child', 'node_tau', 'node_off', 'items')


class SearchTree:
    """A search tree of one ``Solution``.  Arrays: planes [H, n_t+1] unit [n | o]; node_plane [N] (-1: leaf); node_child [N, 2]
    ("+", "-"); node_tau [N, 2] (tau-, tau+); node_off [N+1] with node k's ascending leaf list items[node_off[k]:node_off[k+1]]."""

    def __init__(self, solution, arrays: dict, tol: float, band: Optional[float] = None, stats: Optional[dict] = None):
        self.solution = solution
        self.planes = numpy.ascontiguousarray(arrays['planes'], dtype=numpy.float64)
        self.node_plane = numpy.ascontiguousarray(arrays['node_plane'], dtype=numpy.int32).reshape(-1)
        self.node_child = numpy.ascontiguousarray(arrays['node_child'], dtype=numpy.int32).reshape(-1, 2)
        self.node_tau = numpy.ascontiguousarray(arrays['node_tau'], dtype=numpy.float64).reshape(-1, 2)
        self.node_off = numpy.ascontiguousarray(arrays['node_off'], dtype=numpy.int64).reshape(-1)
        self.items = numpy.ascontiguousarray(arrays['items'], dtype=numpy.int32).reshape(-1)
        self.tol = float(tol)
        self.band = band
        self.stats = dict(stats or {})
        self._rows = None           # host copy of the scan's rows (locate)

    # ---- construction ---------------------------------------------------------------------------------------------------------
    @classmethod
    def build(cls, solution, band: Optional[float] = None, leaf_size: int = 1, max_depth: int = 48, device: int = 0,
              budget: int = 0) -> 'SearchTree':
        """Builds the tree on the device from the locator's rows (the scan's numbers).  ``band`` defaults to 16 tol."""
        tol = float(solution.point_location_tolerance)
        band = 16.0 * tol if band is None else float(band)
        n_t = solution.theta_dim()
        planes, start, plane_of, _ = plane_table(solution.critical_regions, n_t)
        loc = solution.locator(device)
        stats = loc.build_tree(planes, start, plane_of, tol, band, leaf_size, max_depth, budget)
        arrays = loc.get_tree()
        tree = cls(solution, arrays, tol, band, stats)
        loc.tree_owner = tree
        return tree

    @classmethod
    def from_arrays(cls, solution, arrays: dict) -> 'SearchTree':
        """A tree from the arrays of ``to_arrays`` (a tree built earlier, or by another builder)."""
        return cls(solution, arrays, float(arrays['tol']), arrays.get('band'), arrays.get('stats'))

    def to_arrays(self) -> dict:
        out = {k: getattr(self, k).copy() for k in _ARRAYS}
        out['tol'] = self.tol
        if self.band is not None:
            out['band'] = self.band
        return out

    # ---- shape ----------------------------------------------------------------------------------------------------------------
    @property
    def n_nodes(self) -> int:
        return len(self.node_plane)

    def depth(self) -> int:
        d = numpy.zeros(self.n_nodes, dtype=numpy.int64)
        for k in range(self.n_nodes):
            if self.node_plane[k] >= 0:
                d[self.node_child[k]] = d[k] + 1
        return int(d.max()) if len(d) else 0

    def leaf_sizes(self) -> numpy.ndarray:
        leaves = self.node_plane < 0
        return numpy.diff(self.node_off)[leaves]

    # ---- device location ------------------------------------------------------------------------------------------------------
    def _locator(self, device: int):
        loc = self.solution.locator(device)
        if getattr(loc, 'tree_owner', None) is not self:   # a locator holds one tree at a time
            loc.set_tree(self.planes, self.node_plane, self.node_child, self.node_tau, self.node_off, self.items, self.tol)
            loc.tree_owner = self
        return loc

    def locate_batch(self, thetas: numpy.ndarray, inclusive: bool = False, device: int = 0) -> numpy.ndarray:
        """``Solution.get_region_batch`` through the tree: the same indices, bit for bit."""
        sol = self.solution
        if not sol.critical_regions:
            return numpy.full(len(numpy.atleast_2d(thetas)), -1, dtype=numpy.int64)
        return self._locator(device).query(thetas, sol.point_location_tolerance, sol.is_overlapping, want_x=False, inclusive=inclusive,
                                           tree=True)[0]

    def evaluate_batch(self, thetas: numpy.ndarray, inclusive: bool = False, device: int = 0):
        """``Solution.evaluate_batch`` through the tree: (x* [m, n_x], region [m])."""
        sol = self.solution
        th = numpy.atleast_2d(numpy.asarray(thetas, dtype=float))
        if not sol.critical_regions:
            return numpy.full((len(th), 0), numpy.nan), numpy.full(len(th), -1, dtype=numpy.int64)
        region, x = self._locator(device).query(th, sol.point_location_tolerance, sol.is_overlapping, want_x=True, inclusive=inclusive,
                                                tree=True)
        return x, region

    # ---- host location --------------------------------------------------------------------------------------------------------
    def locate(self, theta, inclusive: bool = False, tol: Optional[float] = None) -> int:
        """Host descent (numpy, no device): the index the scan returns for ``theta`` (-1: none)."""
        tol = self.tol if tol is None else float(tol)
        if tol > self.tol:
            raise ValueError(f'query tol {tol} is larger than the tolerance the tree was built for ({self.tol})')
        if self._rows is None:
            ef, row_off, xlaw = self.solution._stacked()
            P = self.solution.program
            self._rows = (ef, row_off, xlaw, getattr(P, 'Q', None), getattr(P, 'c', None), getattr(P, 'H', None))
        ef, row_off, xlaw, Q, c, H = self._rows
        th = numpy.asarray(theta, dtype=numpy.float64).reshape(-1)
        overlapping = bool(self.solution.is_overlapping)
        found, best = -1, numpy.inf
        stack = [0]
        while stack:
            k = stack.pop()
            while self.node_plane[k] >= 0:
                pl = self.planes[self.node_plane[k]]
                s = float(pl[:-1] @ th - pl[-1])
                go_p, go_m = s >= -self.node_tau[k, 0], s <= self.node_tau[k, 1]
                if go_p and go_m:
                    stack.append(int(self.node_child[k, 1]))
                k = int(self.node_child[k, 0] if go_p else self.node_child[k, 1])
            for r in self.items[self.node_off[k]:self.node_off[k + 1]]:
                r = int(r)
                if not overlapping and 0 <= found <= r:
                    break
                rows = ef[row_off[r]:row_off[r + 1]]
                if len(rows) == 0:   # the scan walks rows: a region without rows is never met, here neither
                    continue
                if inclusive:
                    inside = bool(numpy.all(rows[:, 1:] @ th <= rows[:, 0] + tol))
                else:
                    inside = bool(numpy.all(rows[:, 1:] @ th - rows[:, 0] < tol))
                if not inside:
                    continue
                if not overlapping:
                    found = r
                    break
                obj = _objective(xlaw[r], th, Q, c, H)
                if obj < best or (obj == best and r > found):
                    best, found = obj, r
        return found


def _objective(xl, th, Q, c, H) -> float:
    """1/2 x'Qx + theta'H'x + c'x at x = A theta + b (the scan's objective, terms without x dropped)."""
    x = xl[:, 0] + xl[:, 1:] @ th
    g = numpy.zeros_like(x) if c is None else numpy.asarray(c, dtype=float).reshape(-1).copy()
    if H is not None:
        g = g + numpy.asarray(H, dtype=float).reshape(len(x), -1) @ th
    if Q is not None:
        g = g + 0.5 * (numpy.asarray(Q, dtype=float).reshape(len(x), len(x)) @ x)
    return float(g @ x)
