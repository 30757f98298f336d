"""The candidate sweep over bounding boxes and the row screen behind it, on the device (csrc/box_pairs.hpp).

Solution.compare, transition_graph and remove_overlaps start alike: a bounding box per region, the pairs of boxes that overlap, one LP
per listed pair.  This module is the middle step as a device call, under ONE rule for the three callers:

  boxes     [R, 2, n_t], lower bounds then upper bounds, and a usable entry per box.  A NaN lower bound reads as -inf, a NaN upper
            bound as +inf.
  pair      (i, j) is listed iff both boxes are usable and min(hi_a[i, k], hi_b[j, k]) - max(lo_a[i, k], lo_b[j, k]) > margin for every
            coordinate k, in fp64 exactly as written: infinities are ordinary values, an inf - inf that gives NaN fails.
  margin    +tol for compare and remove_overlaps (an overlap of more than tol), -tol for the transition graph (a gap below tol).
  modes     two families: every (i, j), i = j included; one family (box_b None): i < j only.
  order     ascending by (i, j), from counts, an exclusive scan and ordered writes: no sort, and two calls give the same bytes.

  screen    a candidate (i, j) is dropped when one unit row [o | n] of a screened polytope separates it from the box of the other
            side: s = sum_k n_k (lo[k] if n_k > 0 else hi[k]) is the least n.theta on that box, and s - o > 1e-12 (1 + |o|) leaves no
            point of the box inside the row.  Any point common to both sets has n.theta <= o, so a dropped pair has an empty
            intersection as long as each box contains the set it stands for.
"""
from typing import Optional

import numpy

from .._pairs import MAX_DIM, check_pair_indices, check_polytopes

__all__ = ['box_pairs', 'screen_pairs', 'sweep_options', 'SIDES', 'MAX_DIM']

SIDES = {'a': 1, 'b': 2, 'both': 3}     # whose rows are screened (MPC_SCREEN_ROWS_A, MPC_SCREEN_ROWS_B)


def sweep_options(who: str, sweep: str, screen: str):
    """(device sweep?, row screen?) of the ``sweep`` and ``screen`` arguments of compare, transition_graph and remove_overlaps;
    ValueError for any other value, before anything reaches the device."""
    if sweep not in ('host', 'device'):
        raise ValueError(f"{who}: sweep must be 'host' or 'device', not {sweep!r}")
    if screen not in ('none', 'rows'):
        raise ValueError(f"{who}: screen must be 'none' or 'rows', not {screen!r}")
    return sweep == 'device', screen == 'rows'


def _family(who, name, box, usable):
    box = numpy.ascontiguousarray(box, dtype=numpy.float64)
    if box.ndim != 3 or box.shape[1] != 2:
        raise ValueError(f'{who}: {name} must be [R, 2, n_t] (lower bounds, upper bounds), not {list(box.shape)}')
    if box.shape[0] < 1:
        raise ValueError(f'{who}: {name} holds no box')
    if not 1 <= box.shape[2] <= MAX_DIM:
        raise ValueError(f'{who}: n_theta = {box.shape[2]} is outside 1..{MAX_DIM}')
    if usable is None:
        raise ValueError(f'{who}: {name} needs its usable entries')
    usable = numpy.asarray(usable).reshape(-1) != 0
    if len(usable) != len(box):
        raise ValueError(f'{who}: {name} needs one usable entry per box')
    return box, usable


def box_pairs(box_a, usable_a, box_b=None, usable_b=None, margin: float = 0.0, rows=None, count_only: bool = False, device: int = 0,
              cap: Optional[int] = None):
    """The pairs of overlapping boxes (the module docstring): (pair_a, pair_b, stats), int64 and ascending by (i, j).  ``box_b`` None:
    family a against itself, i < j only.  ``rows`` = (i0, i1): only the rows i0 <= i < i1 of family a (a list larger than memory is
    worked through in such chunks).  ``count_only``: the number of pairs of every row of the range, int64 [i1 - i0], and stats, without
    holding a pair.  ``cap``: the room of the first try (default: four pairs per row and 1024); a list that does not fit is not written
    and the call is repeated once with the exact size.  stats: tests, pairs, segments, ms (device), calls.
    ValueError before anything reaches the device for shapes that do not fit, n_theta outside 1..16, an empty family, usable_b without
    box_b, a row range outside the family, a negative cap and a margin that is not finite."""
    from .. import _lib
    who = 'box_pairs'
    ba, ua = _family(who, 'box_a', box_a, usable_a)
    if box_b is None:
        if usable_b is not None:
            raise ValueError(f'{who}: usable_b without box_b (one family against itself takes box_a and usable_a only)')
        bb = ub = None
    else:
        bb, ub = _family(who, 'box_b', box_b, usable_b)
        if bb.shape[2] != ba.shape[2]:
            raise ValueError(f'{who}: the families have different n_theta ({ba.shape[2]} and {bb.shape[2]})')
    if not numpy.isfinite(margin):
        raise ValueError(f'{who}: margin must be finite')
    i0, i1 = (0, len(ba)) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= i0 <= i1 <= len(ba):
        raise ValueError(f'{who}: rows = ({i0}, {i1}) is outside 0 <= i0 <= i1 <= {len(ba)}')
    if cap is not None and int(cap) < 0:
        raise ValueError(f'{who}: cap must be >= 0')
    if count_only:
        _, _, _, counts, stats = _lib.box_pairs(ba, ua, bb, ub, margin, i0, i1, 0, row_counts=True, device=device)
        return counts, dict(stats, calls=1)
    cap = 4 * (i1 - i0) + 1024 if cap is None else int(cap)
    total, pa, pb, _, stats = _lib.box_pairs(ba, ua, bb, ub, margin, i0, i1, cap, device=device)
    calls, ms = 1, stats['ms']
    if total > cap:
        total, pa, pb, _, stats = _lib.box_pairs(ba, ua, bb, ub, margin, i0, i1, total, device=device)
        calls, ms = 2, ms + stats['ms']
    none = numpy.zeros(0, dtype=numpy.int64)
    pa, pb = (none, none.copy()) if not total else (pa[:total], pb[:total])
    return pa, pb, dict(stats, ms=ms, calls=calls)


def screen_pairs(row_off, ef_rows, pair_a, pair_b, box_for_a_rows=None, box_for_b_rows=None, sides: str = 'both', device: int = 0):
    """The row screen of the candidates (pair_a[k], pair_b[k]) of polytopes of unit rows ef_rows = [o | n] in CSR form by row_off (the
    module docstring): (keep, stats), keep a bool mask in candidate order.  ``sides``: 'a' tests the rows of polytope pair_a[k]
    against box_for_a_rows[pair_b[k]], 'b' the rows of polytope pair_b[k] against box_for_b_rows[pair_a[k]], 'both' does both; the box
    tables are [R, 2, n_t], one entry per polytope of the table.  compare and remove_overlaps screen both ways with the regions' boxes;
    the transition graph screens 'b' with the image boxes (there is no box of a preimage).  stats: pairs, dropped, rows_read, ms.
    ValueError before anything reaches the device for shapes that do not fit, n_theta outside 1..16, unknown sides, a missing box
    table and candidate indices out of range."""
    from .. import _lib
    who = 'screen_pairs'
    if sides not in SIDES:
        raise ValueError(f"{who}: sides must be 'a', 'b' or 'both', not {sides!r}")
    off, ef, n_t, R = check_polytopes(who, row_off, ef_rows, max_rows=None)
    pa, pb = check_pair_indices(who, 'pair_a and pair_b', pair_a, pair_b, R)
    boxes = []
    for name, box, bit in (('box_for_a_rows', box_for_a_rows, 1), ('box_for_b_rows', box_for_b_rows, 2)):
        if not SIDES[sides] & bit:
            boxes.append(None)
            continue
        if box is None:
            raise ValueError(f'{who}: sides = {sides!r} needs {name}')
        box = numpy.ascontiguousarray(box, dtype=numpy.float64)
        if box.shape != (R, 2, n_t):
            raise ValueError(f'{who}: {name} must be [{R}, 2, {n_t}], not {list(box.shape)}')
        boxes.append(box)
    if boxes[0] is not None and boxes[1] is not None and box_for_a_rows is box_for_b_rows:
        boxes[1] = boxes[0]      # one table for both sides is uploaded once
    if not len(pa):
        return numpy.zeros(0, dtype=bool), {'pairs': 0, 'dropped': 0, 'rows_read': 0, 'ms': 0.0}
    keep, stats = _lib.pair_screen(off, ef, pa, pb, boxes[0], boxes[1], SIDES[sides], device=device)
    return keep != 0, stats
