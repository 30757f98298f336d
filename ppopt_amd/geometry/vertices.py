"""V-representation of polytopes on the device: ``polytope_vertices(polytopes)`` enumerates the vertices and rays of a batch
of polytopes {x : A x <= b}, one workgroup per polytope (k_region_vertices, csrc/vertices.hpp: the double-description method).
``Solution.vertices()`` does the same for the regions of a solution, from the rows its locator holds."""
from dataclasses import dataclass, field
from typing import List, Sequence, Union

import numpy

from .. import _lib
from .polytope import Polytope

__all__ = ['RegionVertices', 'polytope_vertices', 'vertices_of_rows', 'OK', 'UNBOUNDED', 'NOT_POINTED', 'EMPTY', 'OVERFLOW']

OK, UNBOUNDED, NOT_POINTED, EMPTY, OVERFLOW = (_lib.VX_OK, _lib.VX_UNBOUNDED, _lib.VX_NOT_POINTED, _lib.VX_EMPTY, _lib.VX_OVERFLOW)


@dataclass
class RegionVertices:
    """vertices [V, n] (each polytope's in lexicographic order), offsets [n_poly + 1] into them, incidence [V, 4] uint64 (bit r of word
    r // 64: row r of the polytope is tight, |b_r - a_r v| <= tol (1 + |b_r|)), rays [R, n] (unit 2-norm) with ray_offsets [n_poly + 1],
    status [n_poly] (OK, UNBOUNDED, NOT_POINTED: the rows have rank < n, EMPTY: no interior, OVERFLOW: too many generators) and stats
    (device ms, generators made, the largest intermediate list, merges, overflow repeats)."""
    vertices: numpy.ndarray
    offsets: numpy.ndarray
    incidence: numpy.ndarray
    rays: numpy.ndarray
    ray_offsets: numpy.ndarray
    status: numpy.ndarray
    stats: dict = field(default_factory=dict)

    def __len__(self) -> int:
        return len(self.status)

    def of(self, i: int) -> numpy.ndarray:
        """the vertices of polytope i, [k, n]"""
        return self.vertices[self.offsets[i]:self.offsets[i + 1]]

    def rays_of(self, i: int) -> numpy.ndarray:
        return self.rays[self.ray_offsets[i]:self.ray_offsets[i + 1]]

    def incidence_of(self, i: int) -> numpy.ndarray:
        return self.incidence[self.offsets[i]:self.offsets[i + 1]]


def _slab_bytes(n_t: int, cap: int) -> int:
    """device bytes of one polytope's slab (mpc_region_vertices: two lists of (y, Z), the products and two index lists)"""
    ntk = 4 if n_t <= 4 else 8 if n_t <= 8 else 16
    return cap * (2 * (ntk + 1) * 8 + 2 * 5 * 8 + 8 + 8)


def _check_rows(who: str, row_off, ef, n_t: int, tol: float, max_vertices, slab, budget):
    if not 1 <= n_t <= _lib.VX_MAX_DIM:
        raise ValueError(f'{who}: n_theta = {n_t} must lie in 1..{_lib.VX_MAX_DIM}')
    counts = numpy.diff(row_off)
    if len(counts) and int(counts.max()) > _lib.VX_MAX_ROWS:
        i = int(numpy.argmax(counts))
        raise ValueError(f'{who}: polytope {i} has {int(counts[i])} rows, more than {_lib.VX_MAX_ROWS}')
    if not numpy.all(numpy.isfinite(ef)):
        raise ValueError(f'{who}: the rows must be finite (polytope {int(numpy.searchsorted(row_off, numpy.argwhere(~numpy.isfinite(ef))[0, 0], "right")) - 1})')
    if not (numpy.isfinite(tol) and tol >= 0):
        raise ValueError(f'{who}: tol must be finite and >= 0')
    slab = int(slab) if slab else _lib.VX_DEFAULT_SLAB
    max_slab = int(max_vertices) if max_vertices else _lib.VX_MAX_SLAB
    if not 18 <= slab <= max_slab <= _lib.VX_MAX_SLAB:
        raise ValueError(f'{who}: need 18 <= slab ({slab}) <= max_vertices ({max_slab}) <= {_lib.VX_MAX_SLAB}')
    cap = int(budget) if budget and budget > 0 else _lib.VX_DEFAULT_BUDGET
    if _slab_bytes(n_t, slab) > cap:
        raise ValueError(f'{who}: the budget of {cap} device bytes is too small for one polytope (its slab takes {_slab_bytes(n_t, slab)} bytes)')
    return slab, max_slab


def vertices_of_rows(row_off, ef_rows, n_t: int, tol: float = 1e-9, max_vertices=None, slab=None, budget: int = 0, device: int = 0,
                     who: str = 'polytope_vertices') -> RegionVertices:
    """The V-representation of the polytopes {x : E x <= f} given as stacked [f | E] rows with row offsets (what Solution._stacked and
    polytope_operations._stack build).  max_vertices: the largest generator list a polytope may reach before it stays OVERFLOW (None:
    2^24); slab: the list length of the first pass (None: 256); budget: device bytes of the slabs in flight (<= 0: 4 GiB).  ValueError
    before any launch for n_t outside 1..16, more than 256 rows in a polytope, non-finite rows or a budget too small for one polytope."""
    off = numpy.ascontiguousarray(row_off, dtype=numpy.int64).reshape(-1)
    ef = numpy.ascontiguousarray(ef_rows, dtype=numpy.float64).reshape(-1, int(n_t) + 1)
    slab, max_slab = _check_rows(who, off, ef, int(n_t), tol, max_vertices, slab, budget)
    status, nv, nr, vert, inc, rays, st = _lib.region_vertices(off, ef, int(n_t), tol=tol, slab=slab, max_slab=max_slab, budget=budget,
                                                               device=device)
    offsets = numpy.concatenate([[0], numpy.cumsum(nv)]).astype(numpy.int64)
    ray_offsets = numpy.concatenate([[0], numpy.cumsum(nr)]).astype(numpy.int64)
    stats = {'ms': float(st['ms']), 'generators': int(st['generators']), 'max_list': int(st['max_list']), 'merges': int(st['merges']),
             'repeats': int(st['repeats']), 'overflow': int(st['overflow']), 'launches': int(st['launches']), 'slab': int(st['slab']),
             'status_counts': numpy.bincount(status, minlength=5).tolist()}
    return RegionVertices(vertices=vert, offsets=offsets, incidence=inc, rays=rays, ray_offsets=ray_offsets, status=status, stats=stats)


def polytope_vertices(polytopes: Union[Polytope, Sequence[Polytope]], tol: float = 1e-9, max_vertices=None, device: int = 0, slab=None,
                      budget: int = 0) -> RegionVertices:
    """Vertices (and rays) of every polytope {x : A x <= b} on the device: a RegionVertices (see vertices_of_rows)."""
    plist: List[Polytope] = [polytopes] if isinstance(polytopes, Polytope) else list(polytopes)
    if not plist:
        raise ValueError('polytope_vertices: no polytopes')
    parts = [p.rows() for p in plist]
    n = parts[0].shape[1] - 1
    if any(q.shape[1] - 1 != n for q in parts):
        raise ValueError('polytope_vertices: the polytopes have different dimensions')
    off = numpy.concatenate([[0], numpy.cumsum([len(q) for q in parts])]).astype(numpy.int64)
    return vertices_of_rows(off, numpy.vstack(parts), n, tol=tol, max_vertices=max_vertices, slab=slab, budget=budget, device=device)
