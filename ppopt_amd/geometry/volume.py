"""Volumes and centroids of polytopes on the device: ``polytope_volumes(polytopes)`` runs the vertex pass
(geometry.vertices) and then the boundary triangulation of Cohen & Hickey on the face lattice its incidence masks give
(k_volume_walk, csrc/volume.hpp), one wavefront per (polytope, row).  ``Solution.volumes()`` does the same for the regions of a
solution, ``Solution.coverage_volume()`` compares their sum with the volume of the parameter space."""
from dataclasses import dataclass, field
from typing import List, Sequence, Union

import numpy

from .. import _lib
from .polytope import Polytope
from .vertices import RegionVertices, _check_rows, vertices_of_rows

__all__ = ['RegionVolumes', 'CoverageVolume', 'polytope_volumes', 'volumes_of_rows', 'TOO_LARGE', 'INCONSISTENT', 'STATUS_NAMES']

TOO_LARGE, INCONSISTENT = _lib.VOL_TOO_LARGE, _lib.VOL_INCONSISTENT
STATUS_NAMES = ('OK', 'UNBOUNDED', 'NOT_POINTED', 'EMPTY', 'OVERFLOW', 'TOO_LARGE', 'INCONSISTENT')


@dataclass
class RegionVolumes:
    """volume [P] (0 for EMPTY, +inf for UNBOUNDED and NOT_POINTED, NaN for OVERFLOW, TOO_LARGE and INCONSISTENT), centroid [P, n] (NaN
    unless OK), simplices [P] (of the triangulation; 0 unless OK), status [P] (the vertex pass's OK, UNBOUNDED, NOT_POINTED, EMPTY,
    OVERFLOW, and TOO_LARGE: more than max_simplices simplices or more than 16,384 vertices, INCONSISTENT: the incidence masks do not
    describe a face lattice), stats (device ms, simplices, the largest count of one polytope, launches, polytopes per status) and the
    RegionVertices they were computed from."""
    volume: numpy.ndarray
    centroid: numpy.ndarray
    simplices: numpy.ndarray
    status: numpy.ndarray
    stats: dict = field(default_factory=dict)
    vertices: RegionVertices = None

    def __len__(self) -> int:
        return len(self.status)


@dataclass
class CoverageVolume:
    """total: the summed volume of the OK regions; theta_volume: the volume of {A_t theta <= b_t}; fraction = total / theta_volume;
    status_counts: regions per status name; ok: every region and the parameter space were decided (OK or EMPTY)."""
    total: float
    theta_volume: float
    fraction: float
    status_counts: dict
    ok: bool


def volumes_of_rows(row_off, ef_rows, n_t: int, tol: float = 1e-9, max_simplices=None, max_vertices=None, device: int = 0, budget: int = 0,
                    slab=None, who: str = 'polytope_volumes', vertices: RegionVertices = None) -> RegionVolumes:
    """Volumes and centroids of the polytopes {x : E x <= f} given as stacked [f | E] rows with row offsets: the vertex pass
    (vertices_of_rows; ``vertices``: its result when it has been run already), then the volume pass.  max_simplices: the most simplices
    one polytope may take before it ends TOO_LARGE (None: 2^16); max_vertices, slab and budget as in vertices_of_rows, the budget also
    bounds the bitsets of the volume pass.  ValueError before any launch for n_t outside 1..16, more than 256 rows in a polytope,
    non-finite rows, max_simplices < 1 or a budget too small for one polytope."""
    off = numpy.ascontiguousarray(row_off, dtype=numpy.int64).reshape(-1)
    ef = numpy.ascontiguousarray(ef_rows, dtype=numpy.float64).reshape(-1, int(n_t) + 1)
    _check_rows(who, off, ef, int(n_t), tol, max_vertices, slab, budget)
    cap = _lib.VOL_DEFAULT_MAX_SIMPLICES if max_simplices is None else int(max_simplices)
    if cap < 1:
        raise ValueError(f'{who}: max_simplices = {cap} must be >= 1')
    rv = vertices if vertices is not None else vertices_of_rows(off, ef, int(n_t), tol=tol, max_vertices=max_vertices, slab=slab, budget=budget,
                                                                device=device, who=who)
    limit = int(budget) if budget and budget > 0 else _lib.VOL_DEFAULT_BUDGET
    counts, nv = numpy.diff(off), numpy.diff(rv.offsets)
    need = numpy.where(nv <= _lib.VOL_MAX_VERTS, counts * ((nv + 63) // 64) * 8 + 20 + counts * 8, 0)
    if len(need) and int(need.max()) > limit:
        i = int(numpy.argmax(need))
        raise ValueError(f'{who}: the budget of {limit} device bytes is too small for polytope {i} (its bitsets take {int(need[i])} bytes)')
    volume, centroid, simplices, status, st = _lib.region_volumes(off, ef, int(n_t), rv.offsets, rv.vertices, rv.incidence, rv.status, tol=tol,
                                                                  max_simplices=cap, budget=budget, device=device)
    return RegionVolumes(volume=volume, centroid=centroid, simplices=simplices, status=status, stats=st, vertices=rv)


def polytope_volumes(polytopes: Union[Polytope, Sequence[Polytope]], tol: float = 1e-9, max_simplices=None, max_vertices=None, device: int = 0,
                     budget: int = 0, slab=None) -> RegionVolumes:
    """Volume and centroid of every polytope {x : A x <= b} on the device: a RegionVolumes (see volumes_of_rows)."""
    plist: List[Polytope] = [polytopes] if isinstance(polytopes, Polytope) else list(polytopes)
    if not plist:
        raise ValueError('polytope_volumes: no polytopes')
    parts = [p.rows() for p in plist]
    n = parts[0].shape[1] - 1
    if any(q.shape[1] - 1 != n for q in parts):
        raise ValueError('polytope_volumes: the polytopes have different dimensions')
    off = numpy.concatenate([[0], numpy.cumsum([len(q) for q in parts])]).astype(numpy.int64)
    return volumes_of_rows(off, numpy.vstack(parts), n, tol=tol, max_simplices=max_simplices, max_vertices=max_vertices, device=device,
                           budget=budget, slab=slab)


def coverage_volume(solution, device: int = 0) -> CoverageVolume:
    """Solution.coverage_volume: see there."""
    reduced = getattr(solution, 'overlap_info', None) is not None and not solution.is_overlapping     # pieces share boundaries only
    if not reduced and (solution.is_mixed_integer_sol() or any(r.y_fixation is not None for r in solution.critical_regions)):
        raise ValueError('coverage_volume: mixed-integer solutions are not summed (their regions may overlap)')
    if solution.is_overlapping:
        raise ValueError('coverage_volume: the solution is overlapping (every mpLP solution is): a point may lie in several regions, and '
                         'the sum of their volumes is not a coverage')
    vols = solution.volumes(device=device)
    P = solution.program
    A_t, b_t = numpy.asarray(P.A_t, dtype=float), numpy.asarray(P.b_t, dtype=float).reshape(-1, 1)
    theta = volumes_of_rows([0, len(A_t)], numpy.hstack([b_t, A_t]), A_t.shape[1], device=device, who='Solution.coverage_volume')
    good = vols.status == _lib.VOL_OK
    total = float(vols.volume[good].sum())
    theta_volume = float(theta.volume[0])
    counts = {STATUS_NAMES[k]: int(c) for k, c in enumerate(numpy.bincount(vols.status, minlength=len(STATUS_NAMES))) if c}
    decided = numpy.isin(vols.status, (_lib.VOL_OK, _lib.VOL_EMPTY)).all() and theta.status[0] == _lib.VOL_OK
    fraction = total / theta_volume if theta.status[0] == _lib.VOL_OK and theta_volume > 0 else float('nan')
    return CoverageVolume(total=total, theta_volume=theta_volume, fraction=fraction, status_counts=counts, ok=bool(decided))
