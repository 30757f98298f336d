"""Second moments of polytopes on the device: ``polytope_moments(polytopes)`` runs the vertex pass and then the walk of
geometry.volume with one more sum per wave (k_volume_walk<NT, true>, csrc/volume.hpp), which gives the integral of theta theta^T over
every polytope beside its volume and centroid.  With the three moments the integral of any quadratic over a polytope is host algebra
(``integrate_quadratic``); ``Solution.moments()`` does the same for the regions of a solution, ``Solution.expected_values()`` integrates
the value function and the law over them."""
from dataclasses import dataclass, field
from typing import List, Sequence, Union

import numpy

from .. import _lib
from .polytope import Polytope
from .vertices import RegionVertices, _check_rows, vertices_of_rows
from .volume import STATUS_NAMES

__all__ = ['RegionMoments', 'ExpectedValues', 'polytope_moments', 'moments_of_rows', 'integrate_quadratic']


@dataclass
class RegionMoments:
    """volume [P], centroid [P, n], simplices [P], status [P], stats and vertices as in geometry.volume.RegionVolumes (the same bits), and
    second_moment [P, n, n]: the integral of theta theta^T over the polytope (zeros for EMPTY, NaN for every other status but OK)."""
    volume: numpy.ndarray
    centroid: numpy.ndarray
    second_moment: numpy.ndarray
    simplices: numpy.ndarray
    status: numpy.ndarray
    stats: dict = field(default_factory=dict)
    vertices: RegionVertices = None

    def __len__(self) -> int:
        return len(self.status)

    @property
    def first_moment(self) -> numpy.ndarray:
        """the integral of theta [P, n]: volume * centroid; zeros for EMPTY, NaN for every other status but OK"""
        with numpy.errstate(invalid='ignore'):
            m1 = self.volume[:, None] * self.centroid
        m1[self.status == _lib.VOL_EMPTY] = 0.0
        return m1

    @property
    def covariance(self) -> numpy.ndarray:
        """the covariance of theta uniform on the polytope [P, n, n]: M2 / M0 - c c^T; NaN unless OK"""
        out = numpy.full(self.second_moment.shape, numpy.nan)
        ok = self.status == _lib.VOL_OK
        c = self.centroid[ok]
        out[ok] = self.second_moment[ok] / self.volume[ok, None, None] - c[:, :, None] * c[:, None, :]
        return out


@dataclass
class ExpectedValues:
    """Solution.expected_values: theta uniform on the union of the OK regions.  total: its volume; objective_integral and objective_mean
    (= integral / total) of the value function; x_mean [n_x] and x_cov [n_x, n_x] of the law; theta_mean [n] and theta_cov [n, n];
    objective_integral_by_region and volume_by_region [R] (NaN and the volume pass's values where a region is not OK); status_counts:
    regions per status name; ok: every region was decided (OK or EMPTY)."""
    total: float
    objective_integral: float
    objective_mean: float
    x_mean: numpy.ndarray
    x_cov: numpy.ndarray
    theta_mean: numpy.ndarray
    theta_cov: numpy.ndarray
    objective_integral_by_region: numpy.ndarray
    volume_by_region: numpy.ndarray
    status_counts: dict
    ok: bool


def moments_of_rows(row_off, ef_rows, n_t: int, tol: float = 1e-9, max_simplices=None, max_vertices=None, device: int = 0, budget: int = 0,
                    slab=None, who: str = 'polytope_moments', vertices: RegionVertices = None) -> RegionMoments:
    """Volumes, centroids and second moments of the polytopes {x : E x <= f} given as stacked [f | E] rows with row offsets: the vertex
    pass (``vertices``: its result when it has been run already), then the moment pass.  The arguments and the ValueErrors are those of
    geometry.volume.volumes_of_rows; the budget also bounds the second-moment slots, n_t (n_t + 1) / 2 doubles per row."""
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
    ne = int(n_t) * (int(n_t) + 1) // 2
    need = numpy.where(nv <= _lib.VOL_MAX_VERTS, counts * ((nv + 63) // 64) * 8 + 20 + counts * 8 + counts * ne * 8, 0)
    if len(need) and int(need.max()) > limit:
        i = int(numpy.argmax(need))
        raise ValueError(f'{who}: the budget of {limit} device bytes is too small for polytope {i} (its bitsets and slots take '
                         f'{int(need[i])} bytes)')
    volume, centroid, m2, simplices, status, st = _lib.region_moments(off, ef, int(n_t), rv.offsets, rv.vertices, rv.incidence, rv.status,
                                                                      tol=tol, max_simplices=cap, budget=budget, device=device)
    return RegionMoments(volume=volume, centroid=centroid, second_moment=m2, simplices=simplices, status=status, stats=st, vertices=rv)


def polytope_moments(polytopes: Union[Polytope, Sequence[Polytope]], tol: float = 1e-9, max_simplices=None, max_vertices=None, device: int = 0,
                     budget: int = 0, slab=None) -> RegionMoments:
    """Volume, centroid and second moment of every polytope {x : A x <= b} on the device: a RegionMoments (see moments_of_rows)."""
    plist: List[Polytope] = [polytopes] if isinstance(polytopes, Polytope) else list(polytopes)
    if not plist:
        raise ValueError('polytope_moments: no polytopes')
    parts = [p.rows() for p in plist]
    n = parts[0].shape[1] - 1
    if any(q.shape[1] - 1 != n for q in parts):
        raise ValueError('polytope_moments: the polytopes have different dimensions')
    off = numpy.concatenate([[0], numpy.cumsum([len(q) for q in parts])]).astype(numpy.int64)
    return moments_of_rows(off, numpy.vstack(parts), n, tol=tol, max_simplices=max_simplices, max_vertices=max_vertices, device=device,
                           budget=budget, slab=slab)


def integrate_quadratic(moments: RegionMoments, Q=None, q=None, r=None) -> numpy.ndarray:
    """The integral of 1/2 theta^T Q theta + q^T theta + r over every polytope [P]: 1/2 tr(Q M2) + q^T M1 + r M0.  Q [n, n] or [P, n, n],
    q [n] or [P, n], r a scalar or [P]; a missing coefficient is zero.  NaN where the status is neither OK nor EMPTY."""
    P, n = moments.centroid.shape
    out = numpy.zeros(P)
    known = numpy.isin(moments.status, (_lib.VOL_OK, _lib.VOL_EMPTY))
    m0 = numpy.where(known, moments.volume, 0.0)
    m1 = numpy.where(known[:, None], moments.first_moment, 0.0)
    m2 = numpy.where(known[:, None, None], moments.second_moment, 0.0)
    if Q is not None:
        Q = numpy.asarray(Q, dtype=float)
        if Q.shape not in ((n, n), (P, n, n)):
            raise ValueError(f'integrate_quadratic: Q has shape {Q.shape}, not ({n}, {n}) or ({P}, {n}, {n})')
        out += 0.5 * numpy.einsum('ij,pij->p', Q, m2) if Q.ndim == 2 else 0.5 * numpy.einsum('pij,pij->p', Q, m2)
    if q is not None:
        q = numpy.asarray(q, dtype=float)
        if q.shape not in ((n,), (P, n)):
            raise ValueError(f'integrate_quadratic: q has shape {q.shape}, not ({n},) or ({P}, {n})')
        out += m1 @ q if q.ndim == 1 else numpy.einsum('pi,pi->p', q, m1)
    if r is not None:
        r = numpy.asarray(r, dtype=float)
        if r.shape not in ((), (P,)):
            raise ValueError(f'integrate_quadratic: r has shape {r.shape}, not () or ({P},)')
        out += r * m0
    out[~known] = numpy.nan
    return out


def value_function(solution):
    """Solution.value_function: see there."""
    solution._refuse_merged('value_function')
    P = solution.program
    _, _, xlaw = solution._stacked()
    b, A = xlaw[:, :, 0], xlaw[:, :, 1:]                       # [R, n_x], [R, n_x, n_t]
    n_x, n_t = A.shape[1], A.shape[2]
    Q = numpy.asarray(P.Q, dtype=float) if getattr(P, 'Q', None) is not None else numpy.zeros((n_x, n_x))
    Q = 0.5 * (Q + Q.T)
    H = numpy.asarray(P.H, dtype=float).reshape(n_x, n_t)
    c, c_t = numpy.asarray(P.c, dtype=float).reshape(n_x), numpy.asarray(P.c_t, dtype=float).reshape(n_t)
    Q_t, c_c = numpy.asarray(P.Q_t, dtype=float).reshape(n_t, n_t), float(numpy.asarray(P.c_c, dtype=float).reshape(-1)[0])
    HtA = numpy.einsum('xi,rxj->rij', H, A)
    Qv = numpy.einsum('rxi,xy,ryj->rij', A, Q, A) + HtA + HtA.transpose(0, 2, 1) + Q_t
    qv = numpy.einsum('rxi,xy,ry->ri', A, Q, b) + b @ H + A.transpose(0, 2, 1) @ c + c_t
    rv = 0.5 * numpy.einsum('rx,xy,ry->r', b, Q, b) + b @ c + c_c
    return Qv, qv, rv


def expected_values(solution, max_simplices=None, device: int = 0) -> ExpectedValues:
    """Solution.expected_values: see there."""
    if solution.is_mixed_integer_sol() or any(r.y_fixation is not None for r in solution.critical_regions):
        raise ValueError('expected_values: mixed-integer solutions are not summed (their regions may overlap)')
    if solution.is_overlapping:
        raise ValueError('expected_values: the solution is overlapping (every mpLP solution is): a point may lie in several regions, and '
                         'the sum of their integrals is not an integral over the parameter space')
    solution._refuse_merged('expected_values')
    mom = solution.moments(max_simplices=max_simplices, device=device)
    Qv, qv, rv = value_function(solution)
    by_region = integrate_quadratic(mom, Qv, qv, rv)
    ok = mom.status == _lib.VOL_OK
    _, _, xlaw = solution._stacked()
    b, A = xlaw[ok, :, 0], xlaw[ok, :, 1:]
    m0, m1, m2 = mom.volume[ok], mom.first_moment[ok], mom.second_moment[ok]
    total = float(m0.sum())
    n_t, n_x = mom.centroid.shape[1], xlaw.shape[1]
    nan = float('nan')
    if total > 0:
        theta_mean = m1.sum(axis=0) / total
        theta_cov = m2.sum(axis=0) / total - numpy.outer(theta_mean, theta_mean)
        x1 = numpy.einsum('rxi,ri->x', A, m1) + m0 @ b
        AMb = numpy.einsum('rxi,ri,ry->xy', A, m1, b)
        x2 = numpy.einsum('rxi,rij,ryj->xy', A, m2, A) + AMb + AMb.T + numpy.einsum('r,rx,ry->xy', m0, b, b)
        x_mean = x1 / total
        x_cov = x2 / total - numpy.outer(x_mean, x_mean)
        objective_integral = float(by_region[ok].sum())
        objective_mean = objective_integral / total
    else:
        theta_mean, theta_cov = numpy.full(n_t, nan), numpy.full((n_t, n_t), nan)
        x_mean, x_cov = numpy.full(n_x, nan), numpy.full((n_x, n_x), nan)
        objective_integral, objective_mean = 0.0, nan
    counts = {STATUS_NAMES[k]: int(c) for k, c in enumerate(numpy.bincount(mom.status, minlength=len(STATUS_NAMES))) if c}
    decided = bool(numpy.isin(mom.status, (_lib.VOL_OK, _lib.VOL_EMPTY)).all())
    return ExpectedValues(total=total, objective_integral=objective_integral, objective_mean=objective_mean, x_mean=x_mean, x_cov=x_cov,
                          theta_mean=theta_mean, theta_cov=theta_cov, objective_integral_by_region=by_region, volume_by_region=mom.volume.copy(),
                          status_counts=counts, ok=decided)
