"""The references of the candidate sweep and the row screen (test_box_pairs_cpu.py, test_gpu_box_pairs.py), and the dyadic
boxes both tests run.  Everything is numpy; nothing of ppopt_amd.

The rule: boxes [R, 2, n_t] (lower, upper) with a usable entry each; a NaN lower bound reads as -inf, a NaN upper bound as +inf; the pair
(i, j) is listed iff both are usable and min(hi_a[i, k], hi_b[j, k]) - max(lo_a[i, k], lo_b[j, k]) > margin for every k (a NaN fails).
"""
import numpy

TOL = 2.0 ** -10
SCREEN_EPS = 1e-12


def opened(box):
    """(lo, hi) with NaN bounds opened"""
    box = numpy.asarray(box, dtype=numpy.float64)
    lo, hi = box[:, 0], box[:, 1]
    return numpy.where(numpy.isnan(lo), -numpy.inf, lo), numpy.where(numpy.isnan(hi), numpy.inf, hi)


def overlap_matrix(box_a, box_b):
    """[Ra, Rb, n_t] min(hi) - max(lo) of every pair of boxes, NaN bounds opened"""
    lo_a, hi_a = opened(box_a)
    lo_b, hi_b = opened(box_b)
    with numpy.errstate(invalid='ignore'):
        return numpy.minimum(hi_a[:, None, :], hi_b[None, :, :]) - numpy.maximum(lo_a[:, None, :], lo_b[None, :, :])


def all_pairs(box_a, usable_a, box_b=None, usable_b=None, margin=0.0):
    """(pair_a, pair_b) int64, ascending by (i, j): every pair of the rule; box_b None: one family against itself, i < j only"""
    upper = box_b is None
    if upper:
        box_b, usable_b = box_a, usable_a
    ua, ub = numpy.asarray(usable_a).astype(bool), numpy.asarray(usable_b).astype(bool)
    with numpy.errstate(invalid='ignore'):
        hit = numpy.all(overlap_matrix(box_a, box_b) > margin, axis=2)
    hit &= ua[:, None] & ub[None, :]
    if upper:
        hit &= numpy.triu(numpy.ones(hit.shape, dtype=bool), k=1)
    i, j = numpy.nonzero(hit)
    order = numpy.lexsort((j, i))
    return i[order].astype(numpy.int64), j[order].astype(numpy.int64)


def row_separates(row, box):
    """a unit row [o | n] against a box [2, n_t]: s = sum over ascending k of n_k (lo[k] if n_k > 0 else hi[k]), zero terms skipped, is the
    least n.theta on the box; True when s - o > SCREEN_EPS (1 + |o|)"""
    o, s = float(row[0]), 0.0
    with numpy.errstate(invalid='ignore'):
        for k in range(len(row) - 1):
            n = float(row[1 + k])
            if n > 0.0:
                s = s + n * float(box[0, k])
            elif n < 0.0:
                s = s + n * float(box[1, k])
        return bool(s - o > SCREEN_EPS * (1.0 + abs(o)))


def least_excess(poly, box):
    """max over the rows of s - o (the screen's quantity; > 0: the row separates in exact arithmetic)"""
    out = -numpy.inf
    for row in poly:
        n = row[1:]
        with numpy.errstate(invalid='ignore'):
            s = 0.0
            for k in range(len(n)):
                if n[k] > 0.0:
                    s = s + n[k] * box[0, k]
                elif n[k] < 0.0:
                    s = s + n[k] * box[1, k]
        if s - row[0] > out:
            out = s - row[0]
    return out


def screen(polys, pair_a, pair_b, box_for_a_rows, box_for_b_rows, sides):
    """keep [pairs] bool by the double loop.  sides: 'a' tests the rows of polys[pair_a[k]] against box_for_a_rows[pair_b[k]], 'b' the rows
    of polys[pair_b[k]] against box_for_b_rows[pair_a[k]], 'both' both"""
    keep = numpy.ones(len(pair_a), dtype=bool)
    for k, (i, j) in enumerate(zip(numpy.asarray(pair_a).tolist(), numpy.asarray(pair_b).tolist())):
        if sides in ('a', 'both') and any(row_separates(row, box_for_a_rows[j]) for row in polys[i]):
            keep[k] = False
        elif sides in ('b', 'both') and any(row_separates(row, box_for_b_rows[i]) for row in polys[j]):
            keep[k] = False
    return keep


# ---- boxes that decide every pair exactly -------------------------------------------------------------------------------------------------
def dyadic_boxes(R, n_t, seed):
    """[R, 2, n_t]: lower bounds and widths are multiples of 1/4 (hence of 1/64) in [-4, 4], and a third of the upper bounds is moved by
    +TOL, a third by -TOL: every bound is a multiple of 2^-10 below 8, every difference of two bounds is exact in fp64, and many pairs
    overlap by exactly +TOL or -TOL in some coordinate.  The spread of the lower bounds shrinks with n_t, and
    past n_t = 2 no box is thinner than 1/2, so that pairs exist at n_t = 16."""
    rng = numpy.random.default_rng(seed)
    span = max(2, 24 // n_t)
    lo = rng.integers(-16, -16 + span + 1, size=(R, n_t)) / 4.0
    hi = numpy.minimum(lo + rng.integers(0 if n_t <= 2 else 2, 8, size=(R, n_t)) / 4.0, 4.0)
    hi = hi + rng.integers(-1, 2, size=(R, n_t)) * TOL
    return numpy.stack([lo, hi], axis=1)


def exact_ties(box_a, box_b, margin):
    """the number of pairs whose overlap equals margin exactly in some coordinate"""
    return int(numpy.any(overlap_matrix(box_a, box_b) == margin, axis=2).sum())


def axis_rows(box):
    """the 2 n_t unit rows [o | n] of a finite box [2, n_t]: theta_k <= hi[k], -theta_k <= -lo[k]"""
    n = box.shape[1]
    return numpy.vstack([numpy.column_stack([box[1], numpy.eye(n)]), numpy.column_stack([-box[0], -numpy.eye(n)])])
