"""Operations on polytopes: chord extents, Chebyshev information and uniform sampling by hit-and-run
(reference: geometry/polytope_operations.py).  The chains run on the device (mpc_hit_and_run, csrc/locate.hpp: k_hit_and_run);
DESIGN §3.11 specifies them exactly."""
from typing import List, Optional, Sequence, Union

import numpy

from .. import _lib
from ..critical_region import CriticalRegion
from ..utils.chebyshev_ball import chebyshev_ball
from .polytope import Polytope

# Steps between samples.  Measured with the distribution tests (tests/test_hit_and_run_cpu.py, tests/test_gpu_hit_and_run.py): from
# the Chebyshev centre, the 8-dimensional unit box, simplex and rotated box pass their KS tests after 100 steps, the 10:1 box in 8
# dimensions needs about 1,000 (at 600 steps its KS statistic is 0.9 of the limit with 3,000 chains).
DEFAULT_N_STEPS = 1000
FULL_DIM_RADIUS = 1e-8      # CriticalRegion.is_full_dimension


def get_chebyshev_information(region: CriticalRegion, solver=None):
    """Chebyshev ball of the region {E theta <= f}: SolverOutput with sol = [centre; radius], or None."""
    return chebyshev_ball(*region.get_constraints(), solver=solver)


def find_extents(A, b, d, x) -> float:
    """How far one can move from x along d inside {A x <= b}: min over rows with a_i d > 0 of (b_i - a_i x) / (a_i d); inf when no
    row bounds the ray."""
    A = numpy.asarray(A, dtype=float)
    b = numpy.asarray(b, dtype=float).reshape(-1)
    orth = (A @ numpy.asarray(d, dtype=float).reshape(-1)).reshape(-1)
    point = (A @ numpy.asarray(x, dtype=float).reshape(-1)).reshape(-1)
    dist = float('inf')
    for i in range(A.shape[0]):
        if orth[i] <= 0:
            continue
        dist = min(dist, (b[i] - point[i]) / orth[i])
    return dist


def _stack(polytopes: Sequence[Polytope]):
    """(row_off [P+1], [b | A] rows, n) with the limits of mpc_hit_and_run checked; MpcError before anything touches the device."""
    if not polytopes:
        raise _lib.MpcError('no polytopes')
    parts = []
    for p in polytopes:
        try:
            parts.append(p.rows())
        except ValueError as e:
            raise _lib.MpcError(str(e)) from None
    n = parts[0].shape[1] - 1
    if any(q.shape[1] - 1 != n for q in parts):
        raise _lib.MpcError('the polytopes have different dimensions')
    if not 1 <= n <= _lib.HR_MAX_DIM:
        raise _lib.MpcError(f'hit-and-run needs 1 <= n <= {_lib.HR_MAX_DIM}, got n = {n}')
    worst = max(len(q) for q in parts)
    if worst > _lib.HR_MAX_ROWS:
        raise _lib.MpcError(f'hit-and-run takes at most {_lib.HR_MAX_ROWS} rows per polytope, got {worst}')
    counts = numpy.array([len(q) for q in parts], dtype=numpy.int64)
    return numpy.concatenate([[0], numpy.cumsum(counts)]).astype(numpy.int64), numpy.vstack(parts), n


def chebyshev_centres(row_off, rows, n, device: int = 0):
    """(centres [P, n], radii [P], LP status [P]) of the stacked polytopes: ONE batch of Chebyshev LPs on the device,
    rows padded to the largest polytope (as Solution.chebyshev_centres)."""
    P = len(row_off) - 1
    m = int(numpy.max(numpy.diff(row_off))) + 1
    A = numpy.zeros((P, m, n + 1))
    b = numpy.ones((P, m))
    for i in range(P):
        seg = rows[row_off[i]:row_off[i + 1]]
        k = len(seg)
        A[i, :k, :n] = seg[:, 1:]
        A[i, :k, n] = numpy.linalg.norm(seg[:, 1:], axis=1)
        b[i, :k] = seg[:, 0]
        A[i, k, n] = -1.0          # -r <= 0
        b[i, k] = 0.0
    c = numpy.zeros(n + 1)
    c[n] = -1.0
    status, x, _, _ = _lib.lp_solve_batch(A, b, c, numpy.zeros((P, m), dtype=numpy.uint8), device=device)
    return x[:, :n], numpy.where(status == _lib.LP_OPTIMAL, x[:, n], numpy.nan), status


def hit_and_run_batch(polytopes: Union[Polytope, List[Polytope]], starts: Optional[numpy.ndarray] = None, chains: int = 64,
                      samples: int = 1, n_steps: int = DEFAULT_N_STEPS, seed: int = 0, device: int = 0) -> numpy.ndarray:
    """``chains`` hit-and-run chains in every polytope, ``samples`` samples per chain, one every ``n_steps`` steps.  Returns
    [P, chains, samples, n] ([chains, samples, n] for one Polytope).  ``starts`` [P, n] defaults to the Chebyshev centres.
    Raises MpcError for a polytope that is empty, unbounded or not full dimensional (Chebyshev radius <= 1e-8), and for a start
    outside its polytope; sizes beyond the kernel's limits are refused before the device is touched."""
    single = isinstance(polytopes, Polytope)
    plist = [polytopes] if single else list(polytopes)
    row_off, rows, n = _stack(plist)
    chains, samples, n_steps, seed = int(chains), int(samples), int(n_steps), int(seed)
    if chains < 1 or samples < 1 or n_steps < 1 or samples * n_steps >= 1 << 32:
        raise _lib.MpcError('hit-and-run needs chains >= 1, samples >= 1, n_steps >= 1 and samples * n_steps < 2^32')
    if not 0 <= seed < 1 << 64:
        raise _lib.MpcError('the seed must be a 64-bit unsigned integer')
    # a polytope whose rows do not span R^n contains a line (a slab, say): its chords are finite in almost every direction, so the
    # chains would not stop with MPC_HR_UNBOUNDED -- they would drift along the line
    for i in range(len(plist)):
        seg = rows[row_off[i]:row_off[i + 1], 1:]
        if len(seg) < n or numpy.linalg.matrix_rank(seg) < n:
            raise _lib.MpcError(f'polytope {i} is unbounded (its rows have rank below {n}: it contains a line)')
    if starts is not None:
        starts = numpy.asarray(starts, dtype=numpy.float64)
        if starts.size != len(plist) * n:
            raise _lib.MpcError(f'starts must be [{len(plist)}, {n}], got shape {starts.shape}')
        starts = starts.reshape(len(plist), n)
    else:
        starts, radii, status = chebyshev_centres(row_off, rows, n, device)
        for i, (st, r) in enumerate(zip(status, radii)):
            if st == _lib.LP_INFEASIBLE:
                raise _lib.MpcError(f'polytope {i} is empty')
            if st == _lib.LP_UNBOUNDED:
                raise _lib.MpcError(f'polytope {i} is unbounded (its Chebyshev ball has no largest radius)')
            if not numpy.isfinite(r):
                raise _lib.MpcError(f'the Chebyshev LP of polytope {i} failed (status {int(st)})')
            if r <= FULL_DIM_RADIUS:
                raise _lib.MpcError(f'polytope {i} is not full dimensional (Chebyshev radius {r:.3g})')
    out, status = _lib.hit_and_run(row_off, rows, starts, chains, samples, n_steps, seed, device)
    bad = numpy.argwhere(status != _lib.MPC_HR_OK)
    if len(bad):
        i, k = (int(v) for v in bad[0])
        what = 'is unbounded' if status[i, k] == _lib.MPC_HR_UNBOUNDED else 'does not contain its start point'
        raise _lib.MpcError(f'polytope {i} {what} (chain {k}; {len(bad)} chains stopped)')
    return out[0] if single else out


def hit_and_run(p: Polytope, x_0: numpy.ndarray, n_steps: int = 10, seed: Optional[int] = None) -> numpy.ndarray:
    """One hit-and-run chain of ``n_steps`` steps in p from x_0 (on the device); the end point as [n, 1].  With seed=None the seed
    is drawn from numpy.random.default_rng(), so that the call is unseeded like the reference's."""
    if seed is None:
        seed = int(numpy.random.default_rng().integers(0, 1 << 63))
    x_0 = numpy.asarray(x_0, dtype=numpy.float64).reshape(1, -1)
    return hit_and_run_batch([p], starts=x_0, chains=1, samples=1, n_steps=n_steps, seed=seed)[0, 0, 0].reshape(-1, 1)


def sample_program_theta_space(program, num_samples: int = 10, n_steps: int = DEFAULT_N_STEPS, seed: int = 0,
                               device: int = 0) -> numpy.ndarray:
    """[num_samples, n_theta] points spread uniformly over the program's parameter set {A_t theta <= b_t}: the end points of
    independent hit-and-run chains started at its Chebyshev centre.  MpcError when the set is unbounded or not full dimensional."""
    P = Polytope(numpy.asarray(program.A_t, dtype=float), numpy.asarray(program.b_t, dtype=float))
    try:
        out = hit_and_run_batch(P, chains=num_samples, samples=1, n_steps=n_steps, seed=seed, device=device)
    except _lib.MpcError as e:
        raise _lib.MpcError(f'cannot sample the parameter set A_t theta <= b_t: {e}') from None
    return out[:, 0, :]
