"""The inputs of the law-gap tests (test_compare_cpu.py, test_gpu_compare.py): seeded pairs of partitions of the box [-1, 1]^n with laws,
the padded variants, the hand-made open cases and the hand-built 1-D case.  Everything is numpy and scipy; nothing of ppopt_amd.

A case is a dict: n, K, polys_a, polys_b (lists of [m, n + 1] unit rows [o | n]), laws_a, laws_b ([R, K, n + 1] = [b | A]), and for the
synthetic sets copied (cells of B whose law is a bit-for-bit copy of an A cell's) and shifted (the cell that copies A but not b).
"""
import functools

import numpy
from scipy.optimize import linprog

# n: (depth, K, cells per side, meeting pairs at tol = 1e-8 by the reference radius LP); every shape has 0 knife pairs
SHAPES = {1: (3, 1, 8, 15), 2: (4, 3, 16, 74), 3: (4, 3, 16, 117), 5: (4, 20, 16, 189), 8: (3, 3, 8, 64), 16: (3, 3, 8, 64)}
PAD_TO = 256


def box_rows(n):
    return numpy.vstack([numpy.column_stack([numpy.ones(n), numpy.eye(n)]), numpy.column_stack([numpy.ones(n), -numpy.eye(n)])])


def chebyshev(rows):
    """(centre, radius) of {n.theta <= o}"""
    n = rows.shape[1] - 1
    r = linprog(numpy.append(numpy.zeros(n), -1.0), A_ub=numpy.hstack([rows[:, 1:], numpy.ones((len(rows), 1))]), b_ub=rows[:, 0],
                bounds=[(None, None)] * (n + 1), method='highs-ds')
    assert r.status == 0
    return r.x[:n], float(r.x[n])


def bsp(n, depth, seed):
    """2^depth cells of [-1, 1]^n: at every depth every cell, in order, is cut by a hyperplane with a standard-normal unit normal through
    centre + 0.3 r U(-1, 1)^n, centre and r the cell's Chebyshev centre and radius; the children are the side n.theta <= o, then the other"""
    rng = numpy.random.default_rng(seed)
    cells = [box_rows(n)]
    for _ in range(depth):
        nxt = []
        for c in cells:
            centre, r = chebyshev(c)
            nrm = rng.normal(size=n)
            nrm /= numpy.linalg.norm(nrm)
            o = float(nrm @ (centre + 0.3 * r * rng.uniform(-1.0, 1.0, n)))
            nxt.append(numpy.vstack([c, numpy.append(o, nrm)]))
            nxt.append(numpy.vstack([c, numpy.append(-o, -nrm)]))
        cells = nxt
    return cells


def _holder(polys, point):
    """the first polytope with the point inside"""
    return next(i for i, p in enumerate(polys) if numpy.all(p[:, 1:] @ point <= p[:, 0]))


@functools.lru_cache(maxsize=None)
def synthetic(n):
    """partition A from seed 100 + n, B from 200 + n, standard-normal laws from 300 + n.  Every fourth cell of B (0, 4, ...) copies the
    whole law of the A cell that holds its Chebyshev centre (so the two meet); cell 1 of B copies A of that cell but not b."""
    depth, K, cells, _ = SHAPES[n]
    polys_a, polys_b = bsp(n, depth, 100 + n), bsp(n, depth, 200 + n)
    assert len(polys_a) == len(polys_b) == cells
    rng = numpy.random.default_rng(300 + n)
    laws_a, laws_b = rng.normal(size=(cells, K, n + 1)), rng.normal(size=(cells, K, n + 1))
    copied = {}
    for j in range(0, cells, 4):
        copied[j] = _holder(polys_a, chebyshev(polys_b[j])[0])
        laws_b[j] = laws_a[copied[j]]
    shifted = (1, _holder(polys_a, chebyshev(polys_b[1])[0]))
    laws_b[1, :, 1:] = laws_a[shifted[1], :, 1:]
    return {'n': n, 'K': K, 'polys_a': polys_a, 'polys_b': polys_b, 'laws_a': laws_a, 'laws_b': laws_b, 'copied': copied, 'shifted': shifted}


def pad(poly, rng):
    """the polytope filled to PAD_TO rows by redundant unit rows [|n|_1 + 1 | n]: none touches the box [-1, 1]^n"""
    n = poly.shape[1] - 1
    nrm = rng.normal(size=(PAD_TO - len(poly), n))
    nrm /= numpy.linalg.norm(nrm, axis=1)[:, None]
    return numpy.vstack([poly, numpy.column_stack([numpy.abs(nrm).sum(axis=1) + 1.0, nrm])])


@functools.lru_cache(maxsize=None)
def padded(n):
    """synthetic(n) with every region filled to 256 rows: every pair has 512 rows, the LDS limit"""
    case = dict(synthetic(n))
    rng = numpy.random.default_rng(400 + n)
    case['polys_a'] = [pad(p, rng) for p in case['polys_a']]
    case['polys_b'] = [pad(p, rng) for p in case['polys_b']]
    return case


def table(case):
    """(polys, laws, n_a) of one region table: A's regions, then B's"""
    return case['polys_a'] + case['polys_b'], numpy.concatenate([case['laws_a'], case['laws_b']]), len(case['polys_a'])


def csr(polys):
    return numpy.concatenate([[0], numpy.cumsum([len(p) for p in polys])]).astype(numpy.int64), numpy.vstack(polys)


# ---- hand-made open cases in 2-D --------------------------------------------------------------------------------------------------------
QUADRANT = numpy.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])                                        # theta >= 0
CELL = numpy.array([[2.0, 1.0, 0.0], [-1.0, -1.0, 0.0], [2.0, 0.0, 1.0], [1.0, 0.0, -1.0]])         # [1, 2] x [-1, 2]
HALF_STRIP = numpy.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 1.0]])                     # theta_0 >= 0, 0 <= theta_1 <= 1


def open_quadrant():
    """polytopes [quadrant, cell], K = 1, delta = theta_0 + theta_1 - 1: the quadrant against itself has an unbounded radius; against the
    cell the intersection is [1, 2] x [0, 2], radius 0.5, range [0, 3]"""
    laws = numpy.array([[[-1.0, 1.0, 1.0]], [[0.0, 0.0, 0.0]]])
    return [QUADRANT, CELL], laws, [(0, 0), (0, 1)]


def open_half_strip():
    """polytopes [strip, strip, strip], K = 1, laws theta_0, 0, theta_1: pair (0, 1) has delta = theta_0, range [0, +inf), gap +inf, flag 1;
    pair (2, 1) has delta = theta_1, range [0, 1], gap 1, flag 0.  The radius is 0.5 in both."""
    laws = numpy.array([[[0.0, 1.0, 0.0]], [[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]]])
    return [HALF_STRIP, HALF_STRIP, HALF_STRIP], laws, [(0, 1), (2, 1)]


# ---- the hand-built 1-D case ------------------------------------------------------------------------------------------------------------
def interval(lo, hi):
    return numpy.array([[hi, 1.0], [-lo, -1.0]])


def one_d_by_hand(c):
    """min u^2 s.t. |u| <= 1, |2 theta + u| <= c, worked out by hand: u = 0 on |theta| <= c / 2, u = c - 2 theta on [c / 2, (c + 1) / 2] (where
    2 theta + u = c is active, until u = -1), and mirrored.  (polys, laws [3, 1, 2] = [b | A]) in the order left, middle, right."""
    h, e = c / 2.0, (c + 1.0) / 2.0
    return [interval(-e, -h), interval(-h, h), interval(h, e)], numpy.array([[[-c, -2.0]], [[0.0, 0.0]], [[c, -2.0]]])


def one_d_program_data(c, T=10.0):
    """the matrices A, b, c, H, Q, A_t, b_t, F of that program as an mpQP in u with the parameter |theta| <= T"""
    return {'A': numpy.array([[1.0], [-1.0], [1.0], [-1.0]]), 'b': numpy.array([[1.0], [1.0], [c], [c]]), 'c': numpy.zeros((1, 1)),
            'H': numpy.zeros((1, 1)), 'Q': numpy.array([[2.0]]), 'A_t': numpy.array([[1.0], [-1.0]]), 'b_t': numpy.array([[T], [T]]),
            'F': numpy.array([[0.0], [0.0], [-2.0], [2.0]])}
