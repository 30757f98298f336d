"""The inputs the support-function tests share: the hand cases with their closed forms, and the seeded direction lists
over the polytopes of tests/reduce_cases.py.  No device and no package code: numpy only."""
import numpy

import reduce_cases as rc
from exit_cases import box_rows

COUNTS = (1, 63, 64, 65, 200)      # directions per polytope, in turn: on both sides of any block size up to 64, and several blocks
S2 = numpy.sqrt(2.0)


def hand_cases():
    """[(name, rows, directions, values, statuses)] with status 0 OK, 1 UNBOUNDED, 3 THIN; None: NaN.

      square    [0, 1]^2: the axes, the diagonals (h = the sum of the positive entries), a long and a short direction, and the zero one.
      interval  [-1, 2] at n_theta = 1: h(3) = 6, h(-1/2) = 1/2, h(0) = 0.
      bare      the square again without a direction: it still gets its status and point.
      half      the half-plane x <= 1: +inf across it (every direction but the multiples of +x), h(2 e_x) = 2 along the normal.
      strip     x <= 0, -x <= 0, y <= 1, -y <= 0: radius 0, THIN: NaN for every direction, and no direction LP.
      away      the half-plane x <= -1, which does not hold the origin, where a radius run starts by default: h(2 e_x) = -2.
      cone      x <= -1, y <= -1, away from the origin as well: h(d) = -(d_x + d_y) for d >= 0, +inf otherwise."""
    sq = box_rows([0, 0], [1, 1])
    d_sq = numpy.array([[1.0, 0], [0, 1], [-1, 0], [0, -1], [1, 1], [1, -1], [-1, 1], [-1, -1], [300.0, 400.0], [1e-3, -2e-3], [0, 0]])
    v_sq = [1.0, 1, 0, 0, 2, 1, 1, 0, 700.0, 1e-3, 0]
    iv = numpy.array([[2.0, 1.0], [1.0, -1.0]])
    half = numpy.array([[1.0, 1.0, 0.0]])
    strip = box_rows([0, 0], [0, 1])
    return [('square', sq, d_sq, v_sq, [0] * 11),
            ('interval', iv, numpy.array([[3.0], [-0.5], [0.0]]), [6.0, 0.5, 0.0], [0, 0, 0]),
            ('bare', sq, numpy.zeros((0, 2)), [], []),
            ('half', half, numpy.array([[0.0, 1.0], [-1.0, 0.0], [1.0, 1.0], [2.0, 0.0]]), [numpy.inf, numpy.inf, numpy.inf, 2.0], [1, 1, 1, 0]),
            ('strip', strip, numpy.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]), [None, None, None], [3, 3, 3]),
            ('away', numpy.array([[-1.0, 1.0, 0.0]]), numpy.array([[2.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, 0.0]]), [-2.0, numpy.inf, numpy.inf, 0.0], [0, 1, 1, 0]),
            ('cone', numpy.array([[-1.0, 1.0, 0.0], [-1.0, 0.0, 1.0]]), numpy.array([[1.0, 0.0], [1.0, 1.0], [3.0, 4.0], [-1.0, 0.0], [1.0, -1.0]]),
             [-1.0, -2.0, -7.0, numpy.inf, numpy.inf], [0, 0, 0, 1, 1])]


def directions(rng, rows, count):
    """``count`` directions for the polytope of unit rows ``rows``, shuffled: row normals and their negatives in at most half of the list
    (all 2 m of them where 2 m <= count // 2, a seeded choice of count // 2 otherwise: the optima at duplicated rows are degenerate) and
    Gaussian vectors of norm 10^-3 .. 10^3 in the rest.  So a list of 1 direction holds no normal, the lists of 63 to 65 hold 31 or 32 of
    a polytope's 30 to 208 normals and negatives, a list of 200 holds all of them for the polytopes of up to 50 rows (every polytope of
    n_theta <= 5), and rows300 and rows512 get 100 of their 600 and 1,024."""
    n = rows.shape[1] - 1
    normals = numpy.vstack([rows[:, 1:], -rows[:, 1:]])
    take = rng.permutation(len(normals))[:min(len(normals), count // 2)]
    g = rng.normal(size=(count - len(take), n))
    g *= (10.0 ** rng.uniform(-3.0, 3.0, len(g)) / numpy.linalg.norm(g, axis=1))[:, None]
    d = numpy.vstack([normals[take], g])
    return numpy.ascontiguousarray(d[rng.permutation(len(d))])


SINGLES = {'rows300': rc.rows_300, 'rows512': rc.rows_512}
CASES = list(rc.SETS) + list(SINGLES)
IDS = list(rc.IDS) + list(SINGLES)


def seeded(case):
    """(polys, dirs): the polytopes of a case of reduce_cases and one direction list per polytope, COUNTS in turn (a single polytope: 200)"""
    polys = [SINGLES[case]()] if case in SINGLES else rc.seeded_set(*case)
    rng = numpy.random.default_rng(7000 + (len(polys[0]) if case in SINGLES else case[1]))
    counts = [200] if case in SINGLES else [COUNTS[q % len(COUNTS)] for q in range(len(polys))]
    return polys, [directions(rng, p, c) for p, c in zip(polys, counts)]


def small_q(seed, rows=7):
    """a seeded polygon around the origin of R^2, a tenth of the size of the sets: rows tangent to circles of radius 0.1 .. 0.2"""
    rng = numpy.random.default_rng(seed)
    ang = (numpy.arange(rows) + rng.uniform(-0.2, 0.2, rows)) * 2.0 * numpy.pi / rows
    return numpy.column_stack([rng.uniform(0.1, 0.2, rows), numpy.cos(ang), numpy.sin(ang)])


def scaled_about(rows, centre, factor):
    """the polytope {c + factor (x - c) : x in P} of unit rows: [n.c + factor (o - n.c) | n]"""
    rows = numpy.asarray(rows, dtype=float)
    nc = rows[:, 1:] @ centre
    return numpy.column_stack([nc + factor * (rows[:, 0] - nc), rows[:, 1:]])


ERODE_SEED = 904     # checked on the CPU: with it the reference's erosion and reduction of SETS[1..3] has no knife polytope and no unbounded run
ERODE_SETS, ERODE_IDS = rc.SETS[1:4], rc.IDS[1:4]


def erosion_inputs(case):
    """(polys, E [n, 2], Q): the polytopes of a case of reduce_cases, a seeded map and a seeded small polygon"""
    n = case[0]
    return rc.seeded_set(*case), numpy.random.default_rng(ERODE_SEED + n).normal(size=(n, 2)), small_q(ERODE_SEED + 10 + n)
