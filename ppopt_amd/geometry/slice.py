"""2-D and 1-D slices of polytopes: the polygon or interval of every polytope in a plane or on a line (csrc/locate.hpp:
k_slice_polygons / k_slice_intervals).  Used by Solution.slice_2d / slice_1d and by ppopt_amd.plot."""
from dataclasses import dataclass, field
from typing import List, Sequence

import numpy

from .. import _lib
from .polytope import Polytope


@dataclass
class SolutionSlice:
    """The slice of a batch of regions by the plane theta = theta_0 + U z, clipped to box = (lo0, lo1, hi0, hi1).  Per region:
    ``vertices[k]`` [count, 2] in z, counter-clockwise from the vertex of smallest atan2 about their mean (the reference's
    sort_clockwise order); ``edge_rows[k]`` the row of the region whose edge starts at each vertex (-1 .. -4: the box sides z_0 <= hi0,
    z_1 <= hi1, z_0 >= lo0, z_1 >= lo1); ``areas``; ``status`` (_lib.MPC_SLICE_FULL / EMPTY / LOWDIM, ORed with MPC_SLICE_CUT when a box
    side is an edge)."""
    regions: numpy.ndarray              # [R] region indices (into the solution's critical_regions, or into the polytope list)
    vertices: List[numpy.ndarray] = field(repr=False)
    edge_rows: List[numpy.ndarray] = field(repr=False)
    areas: numpy.ndarray = field(repr=False)
    status: numpy.ndarray = field(repr=False)
    theta_0: numpy.ndarray = field(repr=False)
    U: numpy.ndarray = field(repr=False)
    box: numpy.ndarray = field(repr=False)
    dims: tuple = (0, 1)                # the parameters on the axes (for labels); None for a plane given as (theta_0, U)

    def full(self) -> numpy.ndarray:
        """Mask of the regions whose slice is a full-dimensional polygon (cut by the box or not)."""
        return (self.status & ~_lib.MPC_SLICE_CUT) == _lib.MPC_SLICE_FULL

    def lift(self, z: numpy.ndarray) -> numpy.ndarray:
        """Parameter points theta_0 + U z of plane points z [k, 2]."""
        return numpy.asarray(z, dtype=float).reshape(-1, 2) @ self.U.T + self.theta_0

    def __len__(self):
        return len(self.regions)


@dataclass
class LineSlice:
    """The slice of a batch of regions by the line theta = theta_0 + direction t within t_range: per region the interval [t_a, t_b]
    (NaN for an empty slice), its status (as SolutionSlice.status) and, for solutions, the laws' values x*(theta) at both ends."""
    regions: numpy.ndarray              # [R]
    intervals: numpy.ndarray            # [R, 2]
    status: numpy.ndarray               # [R]
    theta_0: numpy.ndarray = field(repr=False)
    direction: numpy.ndarray = field(repr=False)
    t_range: tuple = (0.0, 1.0)
    x_start: numpy.ndarray = field(default=None, repr=False)    # [R, n_x] at t_a
    x_end: numpy.ndarray = field(default=None, repr=False)      # [R, n_x] at t_b

    def full(self) -> numpy.ndarray:
        """Mask of the regions whose slice is an interval of positive length."""
        return (self.status & ~_lib.MPC_SLICE_CUT) == _lib.MPC_SLICE_FULL

    def __len__(self):
        return len(self.regions)


def _unpack(regions, row_off, vert, edge, count, area, status, theta_0, U, box, dims) -> SolutionSlice:
    starts = row_off[:-1] + 4 * numpy.arange(len(count))
    verts = [vert[s:s + c].copy() for s, c in zip(starts, count)]
    edges = [edge[s:s + c].copy() for s, c in zip(starts, count)]
    return SolutionSlice(regions=numpy.asarray(regions, dtype=numpy.int64), vertices=verts, edge_rows=edges, areas=area, status=status,
                         theta_0=numpy.asarray(theta_0, dtype=float).reshape(-1), U=numpy.asarray(U, dtype=float),
                         box=numpy.asarray(box, dtype=float).reshape(-1), dims=dims)


def slice_rows(row_off, ef_rows, theta_0, U, box, regions=None, eps: float = _lib.SLICE_EPS, device: int = 0, dims=None) -> SolutionSlice:
    """SolutionSlice of stacked [f | E] rows (the layout of Solution._stacked) by one mpc_slice_polygons launch."""
    vert, edge, count, area, status = _lib.slice_polygons(row_off, ef_rows, theta_0, U, box, eps, device)
    if regions is None:
        regions = numpy.arange(len(count))
    return _unpack(regions, numpy.asarray(row_off, dtype=numpy.int64), vert, edge, count, area, status, theta_0, U, box, dims)


def slice_polytopes(polytopes: Sequence[Polytope], theta_0, U, box, eps: float = _lib.SLICE_EPS, device: int = 0) -> SolutionSlice:
    """The slice of every polytope {A x <= b} by the plane x = theta_0 + U z within box = (lo0, lo1, hi0, hi1): one device launch.
    MpcError before any launch for polytopes of different dimensions or beyond the kernel's limits (n <= 64, <= 256 rows)."""
    if not polytopes:
        raise _lib.MpcError('no polytopes')
    parts = []
    for p in polytopes:
        try:
            parts.append(p.rows())
        except ValueError as e:
            raise _lib.MpcError(str(e)) from None
    if any(q.shape[1] != parts[0].shape[1] for q in parts):
        raise _lib.MpcError('the polytopes have different dimensions')
    row_off = numpy.concatenate([[0], numpy.cumsum([len(q) for q in parts])]).astype(numpy.int64)
    return slice_rows(row_off, numpy.vstack(parts), theta_0, U, box, eps=eps, device=device)
