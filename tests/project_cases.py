"""The inputs the projection tests share: the hand cases, whose answers are derived in the docstrings, and the seeded
polytopes.  No device and no package code: numpy only."""
import itertools

import numpy

from exit_cases import box_rows
from reduce_cases import polytope

TOL = 1e-6           # every comparison against the reference runs here: an exact-zero radius is far outside the knife band
OK, THIN, WHOLE, TOO_LARGE = range(4)
S2, S3 = numpy.sqrt(2.0), numpy.sqrt(3.0)


def _unit(o, *n):
    n = numpy.asarray(n, dtype=float)
    s = numpy.linalg.norm(n)
    return numpy.append(o / s, n / s)


def octahedron():
    """|x| + |y| + |z| <= 1: the eight rows (sx x + sy y + sz z <= 1) / sqrt 3, signs in the order of itertools.product((1, -1))"""
    return numpy.array([_unit(1.0, *s) for s in itertools.product((1.0, -1.0), repeat=3)])


def opposing(k=24):
    """2 k rows tangent to the unit circle in the plane: k with a positive coefficient of y, then k with a negative one"""
    ang = (numpy.arange(k) + 0.5) * numpy.pi / k
    up = numpy.column_stack([numpy.ones(k), numpy.cos(ang), numpy.sin(ang)])
    return numpy.vstack([up, up * numpy.array([1.0, 1.0, -1.0])])


def hand_cases():
    """[(name, rows, n_elim, status, result rows or None, peak)]: the trailing n_elim coordinates go, the last one first.

      square      x <= 1, y <= 1, -x <= 0, -y <= 0 without y.  Z: x <= 1, -x <= 0.  P: y <= 1, N: -y <= 0, their combination is
                  0 <= 1: dropped.  [0, 1] as x <= 1, -x <= 0; 3 raw rows.  (On a line the run of either end is unbounded: kept, wide.)
      triangle_x  the triangle (0, 0), (2, 0), (1, 1): -y <= 0, (x + y <= 2) / sqrt 2, (-x + y <= 0) / sqrt 2, without y.  P: rows 1
                  and 2, N: row 0.  (1) row_1 + (1 / sqrt 2) row_0 = [sqrt 2 | 1 / sqrt 2] -> x <= 2; row_2 likewise -> -x <= 0.
      triangle_y  the same triangle in (y, x), without x.  Z: -y <= 0.  P: x + y <= 2, N: -x + y <= 0: their sum is 2 y <= 2, scaled
                  y <= 1.  [0, 1] as -y <= 0, y <= 1.
      simplex     -x <= 0, -y <= 0, -z <= 0, (x + y + z <= 1) / sqrt 3 without z.  Z: the first two.  (1) row_3 + (1 / sqrt 3) row_2 =
                  (x + y <= 1) / sqrt 3, scaled (x + y <= 1) / sqrt 2.  The triangle of 3 rows.
      octahedron  without z.  P: the four rows with + z, N: the four with - z, Z empty: 16 raw rows.  Equal signs of x and of y:
                  (2 sx x + 2 sy y <= 2) / 3, the side (sx x + sy y <= 1) / sqrt 2 of the diamond, once for every p.  Equal signs of
                  x alone: sx x <= 1, twice (as are sy y <= 1): it meets the diamond in a vertex, the set beyond it is flat: removed,
                  the first copy against the second, the second on its own.  Opposite signs of both: 0 <= 2 / 3, dropped.  The diamond
                  of 4 rows in the order of P.
      strip       0 <= y <= 1 in (y, x) without x: both rows are Z, P and N are empty.  [0, 1] from Z alone.
      half_plane  (x + y <= 1) / sqrt 2 without y: P has the row, N and Z are empty: no rows are left, the whole line.
      empty       x <= 0, -x <= -1 in (y, x) without x: the combination of the two is 0 <= -1, the set is empty.  The thin test sees
                  that first (the radius is -1/2); eliminate() of the reference, which runs no thin test, reports the zero combination.
      flat        x <= 0, -x <= 0, y <= 1, -y <= 0 without y: radius 0, THIN.
      product     24 rows with a positive and 24 with a negative coefficient of y, tangent to the unit circle, without y:
                  24 * 24 = 576 > 512 rows."""
    sq = box_rows([0, 0], [1, 1])
    tri = numpy.array([_unit(0.0, 0, -1), _unit(2.0, 1, 1), _unit(0.0, -1, 1)])
    simplex = numpy.array([_unit(0.0, -1, 0, 0), _unit(0.0, 0, -1, 0), _unit(0.0, 0, 0, -1), _unit(1.0, 1, 1, 1)])
    diamond = numpy.array([_unit(1.0, sx, sy) for sx, sy, sz in itertools.product((1.0, -1.0), repeat=3) if sz > 0])
    return [('square', sq, 1, OK, numpy.array([[1.0, 1.0], [0.0, -1.0]]), 3),
            ('triangle_x', tri, 1, OK, numpy.array([[2.0, 1.0], [0.0, -1.0]]), 2),
            ('triangle_y', tri[:, [0, 2, 1]], 1, OK, numpy.array([[0.0, -1.0], [1.0, 1.0]]), 2),
            ('simplex', simplex, 1, OK, numpy.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], _unit(1.0, 1, 1)]), 3),
            ('octahedron', octahedron(), 1, OK, diamond, 16),
            ('strip', numpy.array([[1.0, 1.0, 0.0], [0.0, -1.0, 0.0]]), 1, OK, numpy.array([[1.0, 1.0], [0.0, -1.0]]), 2),
            ('half_plane', _unit(1.0, 1, 1)[None], 1, WHOLE, None, 0),
            ('empty', numpy.array([[0.0, 0.0, 1.0], [-1.0, 0.0, -1.0]]), 1, THIN, None, 0),
            ('flat', box_rows([0, 0], [0, 1]), 1, THIN, None, 0),
            ('product', opposing(24), 1, TOO_LARGE, None, 576)]


def octagon():
    """the unit square [0, 1]^2 + the diamond |x| + |y| <= 1: the square's sides pushed out by 1 (x <= 2, y <= 2, -x <= 1, -y <= 1) and
    the diamond's sides pushed out by the square's support (sx x + sy y <= 1 + max(sx, 0) + max(sy, 0)): 8 rows [o | n], not scaled"""
    rows = [[2.0, 1, 0], [2.0, 0, 1], [1.0, -1, 0], [1.0, 0, -1]]
    rows += [[1.0 + max(sx, 0) + max(sy, 0), sx, sy] for sx, sy in itertools.product((1.0, -1.0), repeat=2)]
    return numpy.array(rows)


def seeded_set(n, n_elim, tangent, k, seed):
    """k polytopes at dimension n: the box c +- 2 around a centre uniform in [-1, 1]^n and ``tangent`` rows with normals uniform on the
    sphere at distance 0.5 to 1 from c, shuffled"""
    rng = numpy.random.default_rng(seed)
    return [polytope(rng, n, tangent, 0, 0) for _ in range(k)]


# (n, n_elim, tangent rows, polytopes, seed); the seeds were checked on the CPU: the reference alone reports no knife polytope and every
# nonzero combination norm is at least 1e-4 (tests/test_project_cpu.py checks the small ones again)
SETS = [(2, 1, 6, 12, 60), (3, 1, 10, 12, 61), (3, 2, 10, 12, 62), (4, 2, 8, 8, 63), (5, 2, 8, 6, 64), (6, 3, 6, 4, 65)]
IDS = [f'n{c[0]}e{c[1]}' for c in SETS]
WIDE_DIM = (16, 1, 30, 2, 66)     # n = 16: the widest rows, LDS for 512 rows of 16 coordinates
MANY_ROWS = (5, 1, 34, 1, 67)     # one step of more than 256 raw rows: mask words past the fourth, LDS above 48 KB
