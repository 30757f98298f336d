"""The host side that the pair-stage calls share (overlap.py, transition.py, compare.py, exit_sets.py, and the checks of _cells.py,
geometry/reduce.py and geometry/box_pairs.py): the limits, the argument checks, the feasible-point prologue, the box
sweep on the host and the whole candidate stage between the boxes and the pair kernel.  Host only: nothing here imports the library
at module level; feasible_points, and candidate_pairs with sweep='device' or screen='rows', import what they call inside.

The three host sweeps are ONE core (sweep_boxes) behind a NaN rule, a preparation of the boxes that candidate_pairs applies before
either sweep, the host's or the device's:

  'mask'        overlap.box_pairs: a box that holds a NaN meets nothing, so it is not usable.
  'bound'       compare.cross_box_pairs, and the rule of geometry.box_pairs: a NaN lower bound reads as -inf, a NaN upper bound as +inf.
  'coordinate'  transition.image_box_pairs: BOTH bounds of a coordinate are opened where either is NaN, and a coordinate difference that
                is NaN (inf - inf) passes on the host; on the device it fails, which no box of a usable region shows.
"""
import time

import numpy

MAX_DIM = 16      # n_theta of the device kernels
MAX_ROWS = 256    # rows of a region or a polytope of the pair stage (MERGE_MAX_ROWS of _lib.py)


# ---- argument checks: every ValueError in the name of ``who``, before anything reaches the device ------------------------------------------
def check_scalars(who, n_t, tol=None):
    if not (isinstance(n_t, (int, numpy.integer)) and 1 <= n_t <= MAX_DIM):
        raise ValueError(f'{who}: n_theta = {n_t} is outside 1..{MAX_DIM}')
    if tol is not None and not (numpy.isfinite(tol) and tol >= 0.0):
        raise ValueError(f'{who}: tol must be finite and >= 0')


def check_polytopes(who, row_off, ef_rows, n_t=None, tol=None, max_rows=MAX_ROWS, extra=(), word=None):
    """(off int64 [R + 1], ef float64 [rows, n_t + 1], n_t, R) of polytopes of unit rows ef_rows = [o | n] in CSR form by row_off.  The
    refusals, in this order: n_theta outside 1..16 and, when given, tol (check_scalars); the shapes; 1..max_rows rows per polytope; a
    non-finite entry.  ``extra``: dense arrays with one entry per polytope as (label, array, shape of an entry); the label ('Phi [R, n_t,
    n_t]') stands in the shape refusal and ``word`` ('maps') in 'rows and maps must be finite'.  ``n_t`` None: it is read from ef_rows,
    which must then be [rows, n_t + 1] already (law_gap_pairs, screen_pairs).  ``max_rows`` None: the shapes only.  A caller with
    refusals of its own between two of these makes two calls, check_scalars being the first."""
    off = numpy.ascontiguousarray(row_off, dtype=numpy.int64).reshape(-1)
    R = len(off) - 1
    if n_t is None:
        ef = numpy.ascontiguousarray(ef_rows, dtype=numpy.float64)
        if ef.ndim != 2 or ef.shape[1] < 2 or R < 1 or off[0] != 0 or off[-1] != len(ef):
            raise ValueError(f'{who}: row_off [R + 1] must run from 0 to the number of rows of ef_rows [rows, n_t + 1] and describe R >= 1 polytopes')
        n_t = ef.shape[1] - 1
        check_scalars(who, n_t, tol)
    else:
        check_scalars(who, n_t, tol)
        ef = numpy.ascontiguousarray(ef_rows, dtype=numpy.float64).reshape(-1, n_t + 1)
        if R < 1 or off[0] != 0 or off[-1] != len(ef) or any(numpy.shape(a) != (R,) + tuple(entry) for _, a, entry in extra):
            labels = ['row_off [R + 1]'] + [label for label, _, _ in extra]
            named = ' and '.join(filter(None, [', '.join(labels[:-1]), labels[-1]]))      # 'row_off [R + 1], Phi [..] and phi [..]'
            raise ValueError(f'{who}: {named} must describe R >= 1 polytopes')
    if max_rows is not None:
        check_rows_finite(who, off, [ef] + [a for _, a, _ in extra], max_rows, word)
    return off, ef, n_t, R


def map_entries(Phi, phi, n_t):
    """the ``extra`` of check_polytopes for the maps theta+ = Phi_i theta + phi_i (its ``word`` is 'maps')"""
    return [('Phi [R, n_t, n_t]', Phi, (n_t, n_t)), ('phi [R, n_t]', phi, (n_t,))]


def check_rows_finite(who, off, arrays, max_rows=MAX_ROWS, word=None):
    """the last two refusals of check_polytopes, for a caller that has its own before them"""
    counts = numpy.diff(off)
    if counts.min() < 1 or counts.max() > max_rows:
        raise ValueError(f'{who}: every polytope needs 1..{max_rows} rows')
    if not all(numpy.all(numpy.isfinite(a)) for a in arrays):
        raise ValueError(f"{who}: rows{' and ' + word if word else ''} must be finite")


def check_pair_indices(who, names, pair_a, pair_b, R):
    """(pair_a, pair_b) as int64 vectors; ``names`` ('pair_a and pair_b') is the caller's word for them in the refusal."""
    pa = numpy.ascontiguousarray(pair_a, dtype=numpy.int64).reshape(-1)
    pb = numpy.ascontiguousarray(pair_b, dtype=numpy.int64).reshape(-1)
    if pa.shape != pb.shape or (len(pa) and (min(pa.min(), pb.min()) < 0 or max(pa.max(), pb.max()) >= R)):
        raise ValueError(f'{who}: {names} must be two index arrays of one length into the polytopes')
    return pa, pb


def check_region_limits(who, regions, n_t, of=''):
    """The limits of the device on a solution's regions: n_theta, then the rows of every region ('region 3 of this solution has ...'
    with ``of`` = 'of this solution').  A caller with a refusal between the two passes no regions first."""
    if n_t > MAX_DIM:
        raise ValueError(f'{who}: n_theta = {n_t} > {MAX_DIM}')
    for i, r in enumerate(regions):
        if numpy.asarray(r.E).reshape(-1, n_t).shape[0] > MAX_ROWS:
            raise ValueError(f"{who}: region {i}{of and ' ' + of} has more than {MAX_ROWS} rows")


# ---- the prologue of every pair-stage call ---------------------------------------------------------------------------------------------------
def feasible_points(off, ef, void=(), device: int = 0):
    """(xs [R, n_t], box [R, 2, n_t], usable [R], stats) by one _lib.merge_regions: a feasible point (0 where the device found none) and
    the bounding box of every polytope; usable: the device found it non-empty and it is not among ``void``."""
    from . import _lib
    xs, box, status, stats = _lib.merge_regions(off, ef, device)
    usable = status == 0
    usable[list(void)] = False
    return numpy.where(numpy.isfinite(xs), xs, 0.0), box, usable, stats


# ---- the candidate stage -----------------------------------------------------------------------------------------------------------------------
def _masked(box, usable):
    return box, usable & ~numpy.isnan(box).any(axis=(1, 2))


def _open_bounds(box, usable):
    if not numpy.isnan(box).any():
        return box, usable
    return numpy.stack([numpy.where(numpy.isnan(box[:, 0]), -numpy.inf, box[:, 0]), numpy.where(numpy.isnan(box[:, 1]), numpy.inf, box[:, 1])], axis=1), usable


def _open_coordinates(box, usable):
    unknown = numpy.isnan(box).any(axis=1)
    if not unknown.any():
        return box, usable
    box = box.copy()
    box[:, 0][unknown], box[:, 1][unknown] = -numpy.inf, numpy.inf
    return box, usable


NAN_RULES = {'mask': (_masked, False), 'bound': (_open_bounds, False), 'coordinate': (_open_coordinates, True)}     # (preparation, a NaN difference passes)


def sweep_boxes(lo, hi, owner, family, margin: float, nan_passes: bool = False):
    """The pairs of the boxes [lo[k], hi[k]] (each [N, n_t]) that overlap by more than ``margin`` in every coordinate, as (owner of one,
    owner of the other), int64 and ascending: a sweep along the first coordinate.  ``family`` None: one family, every pair once with the
    smaller owner first.  ``family`` [N] bool: pairs of a True box and a False box only, the True one's owner first.  ``nan_passes``: a
    coordinate whose difference is NaN does not fail the pair."""
    order = numpy.argsort(lo[:, 0], kind='stable')
    lo, hi, owner = lo[order], hi[order], owner[order]
    if family is not None:
        family = family[order]
        first = family.tolist()
    end = numpy.searchsorted(lo[:, 0], hi[:, 0] - margin, side='left').tolist()    # lo_l < hi_k - margin for l in (k, end[k])
    at, found = [], []      # the boxes k with a hit, and per k the owners of the boxes after it that it meets
    with numpy.errstate(invalid='ignore'):
        for k in range(len(owner) - 1):
            e = end[k]
            if e <= k + 1:
                continue
            if family is None:
                other = slice(k + 1, e)
            else:
                other = numpy.flatnonzero(family[k + 1:e] != first[k]) + k + 1
                if not len(other):
                    continue
            depth = numpy.minimum(hi[k], hi[other]) - numpy.maximum(lo[k], lo[other])
            hit = ~numpy.any(depth <= margin, axis=1) if nan_passes else numpy.all(depth > margin, axis=1)
            at.append(k)
            found.append(owner[other][hit])
    if not found:
        return numpy.zeros(0, dtype=numpy.int64), numpy.zeros(0, dtype=numpy.int64)
    counts = [len(f) for f in found]
    mine, other = numpy.repeat(owner[at], counts), numpy.concatenate(found)
    if family is None:
        pa, pb = numpy.minimum(mine, other), numpy.maximum(mine, other)
    else:
        swap = numpy.repeat(~family[at], counts)
        pa, pb = numpy.where(swap, other, mine), numpy.where(swap, mine, other)
    o = numpy.lexsort((pb, pa))
    return pa[o].astype(numpy.int64), pb[o].astype(numpy.int64)


def host_pairs(rule: str, box_a, usable_a, box_b, usable_b, margin: float):
    """The host sweep under a NaN rule of the module docstring: the usable boxes of box_a [Ra, 2, n_t] (lower, upper) against those of
    box_b, every (i, j); ``box_b`` None: box_a against itself, i < j only."""
    prepare, nan_passes = NAN_RULES[rule]
    box_a, usable_a = prepare(box_a, usable_a)
    ia = numpy.flatnonzero(usable_a)
    if box_b is None:
        return sweep_boxes(box_a[ia, 0], box_a[ia, 1], ia, None, margin, nan_passes)
    box_b, usable_b = prepare(box_b, usable_b)
    ib = numpy.flatnonzero(usable_b)
    return sweep_boxes(numpy.concatenate([box_a[ia, 0], box_b[ib, 0]]), numpy.concatenate([box_a[ia, 1], box_b[ib, 1]]), numpy.concatenate([ia, ib]),
                       numpy.arange(len(ia) + len(ib)) < len(ia), margin, nan_passes)


def candidate_pairs(who, rule, box_a, usable_a, box_b, usable_b, margin, off, ef, screen_boxes, sides, sweep='host', screen='none', device=0, shift=0):
    """The step between the boxes and the pair kernel for partition_by_value, transition_pairs and compare_solutions: (pair_a, pair_b,
    stats).  The sweep is host_pairs(rule, ...), or with ``sweep`` = 'device' geometry.box_pairs on the boxes the rule has prepared, the
    same list.  ``screen`` = 'rows': geometry.screen_pairs then drops the candidates that a row separates from the partner's box;
    ``screen_boxes()`` gives its two box tables (it is called inside the screen's time) and ``sides`` whose rows are tested; polytope j of
    family b is polytope j + ``shift`` of the table (off, ef).  stats: sweep_ms, the wall time of the sweep; sweep_kernel_ms with the device
    sweep; box_candidates, screened, screen_kernel_ms and screen_ms (wall) with the screen."""
    from .geometry.box_pairs import box_pairs, screen_pairs, sweep_options
    on_device, rows_screen = sweep_options(who, sweep, screen)
    stats = {}
    t0 = time.perf_counter()
    if on_device:
        prepare = NAN_RULES[rule][0]
        family_b = (None, None) if box_b is None else prepare(box_b, usable_b)
        pa, pb, sw = box_pairs(*prepare(box_a, usable_a), *family_b, margin=margin, device=device)
        stats['sweep_kernel_ms'] = sw['ms']
    else:
        pa, pb = host_pairs(rule, box_a, usable_a, box_b, usable_b, margin)
    stats['sweep_ms'] = (time.perf_counter() - t0) * 1e3
    if rows_screen:
        t0 = time.perf_counter()
        keep, sc = screen_pairs(off, ef, pa, pb + shift, *screen_boxes(), sides=sides, device=device)
        stats.update(box_candidates=len(pa), screened=int(sc['dropped']), screen_kernel_ms=sc['ms'])
        pa, pb = pa[keep], pb[keep]
        stats['screen_ms'] = (time.perf_counter() - t0) * 1e3
    return pa, pb, stats
