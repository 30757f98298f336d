"""The inputs the row-reduction tests share: the hand cases, whose masks are derived in the docstrings, the seeded
polytopes, and the region difference whose children exceed 256 rows.  No device and no package code: numpy only."""
import numpy

from exit_cases import box_rows

TOL = 1e-6           # every comparison against the reference runs here: an exact-zero radius is far outside the knife band


def _unit(o, *n):
    n = numpy.asarray(n, dtype=float)
    s = numpy.linalg.norm(n)
    return numpy.append(o / s, n / s)


def hand_cases():
    """[(name, rows, kept, thin)]; the unit square is x <= 1, y <= 1, -x <= 0, -y <= 0 in this order, the extra row comes last.

      outside   x <= 2: the square with x >= 2 is empty: removed.  Every side of the square bounds it: kept.
      touching  x + y <= 2 meets the square in the vertex (1, 1) only: the set beyond it has radius 0: removed.
      cutting   x + y <= 3/2 cuts the corner off: kept; beyond x <= 1 the triangle (1, 0), (3/2, 0), (1, 1/2) is left: every side kept.
      twice     x <= 1 first and last: when row 0 is tested the copy is still live and the set beyond is flat: removed; when the copy is
                tested row 0 is gone and the strip 1 <= x beyond it is unbounded to the right only in x, its radius is 1/2: kept.
      interval  [0, 1] as x <= 1, -x <= 0, then x <= 3, n_theta = 1: removed.  (The run of -x <= 0 meets upper bounds only and is unbounded:
                kept, and counted as wide.)
      flat      x <= 0, -x <= 0, y <= 1, -y <= 0: radius 0, THIN: unchanged, no row tested."""
    sq = box_rows([0, 0], [1, 1])
    return [('outside', numpy.vstack([sq, _unit(2.0, 1, 0)]), [1, 1, 1, 1, 0], False),
            ('touching', numpy.vstack([sq, _unit(2.0, 1, 1)]), [1, 1, 1, 1, 0], False),
            ('cutting', numpy.vstack([sq, _unit(1.5, 1, 1)]), [1, 1, 1, 1, 1], False),
            ('twice', numpy.vstack([sq, sq[0]]), [0, 1, 1, 1, 1], False),
            ('interval', numpy.array([[1.0, 1.0], [0.0, -1.0], [3.0, 1.0]]), [1, 1, 0], False),
            ('flat', box_rows([0, 0], [0, 1]), [1, 1, 1, 1], True)]


def polytope(rng, n, tangent, outside, copies, box=True):
    """One bounded polytope of unit rows [o | n] around a random centre c, shuffled: the box c +- 2 (2 n rows, when ``box``), ``tangent``
    rows at distance 0.5 to 1 from c, ``outside`` rows at distance 2 sqrt(n) + (0.5 to 1.5), beyond every corner of the box and so
    strictly redundant, and ``copies`` exact copies of rows drawn from the ones before."""
    c = rng.uniform(-1.0, 1.0, n)
    parts = [box_rows(c - 2.0, c + 2.0)] if box else []
    for count, lo, hi in ((tangent, 0.5, 1.0), (outside, 2.0 * numpy.sqrt(n) + 0.5, 2.0 * numpy.sqrt(n) + 1.5)):
        N = rng.normal(size=(count, n))
        N /= numpy.linalg.norm(N, axis=1, keepdims=True)
        parts.append(numpy.column_stack([N @ c + rng.uniform(lo, hi, count), N]))
    rows = numpy.vstack(parts)
    rows = numpy.vstack([rows, rows[rng.integers(0, len(rows), copies)]])
    return rows[rng.permutation(len(rows))]


def seeded_set(n, seed, k, rows=(15, 40)):
    """k polytopes of rows[0] .. rows[1] rows at n_theta = n: about a tenth of the rows outside, a tenth copies, the rest tangent"""
    rng = numpy.random.default_rng(seed)
    out = []
    for _ in range(k):
        m = int(rng.integers(rows[0], rows[1] + 1))
        outside, copies = max(1, m // 10), max(1, m // 10)
        out.append(polytope(rng, n, m - 2 * n - outside - copies, outside, copies))
    return out


# (n_theta, seed, polytopes, (fewest, most) rows); the seeds were checked on the CPU: the reference alone reports no knife polytope and no
# unbounded run (tests/test_reduce_cpu.py checks the small ones again).  An unbounded run is a legitimate outcome (the set beyond the only
# upper bound of an interval, say); these sets are chosen to have none so that "none wide" can be asserted of the device.
SETS = [(1, 44, 6, (15, 40)), (2, 42, 12, (15, 40)), (3, 43, 24, (15, 40)), (5, 45, 40, (15, 40)), (16, 46, 4, (96, 104))]
IDS = [f'n{c[0]}' for c in SETS]


def rows_300(seed=47):
    """one polytope of 300 rows at n_theta = 2: its kept mask uses the words 0 to 4, its rows reach past word 4"""
    return polytope(numpy.random.default_rng(seed), 2, 250, 30, 16)


def rows_512(seed=48):
    """one polytope of 512 rows at n_theta = 16, 384 tangent and 128 outside, no box: 78,840 bytes of LDS"""
    return polytope(numpy.random.default_rng(seed), 16, 384, 128, 0, box=False)


def many_rows_difference(n_source=200, n_target=100, seed=49):
    """(polys, Phi, phi, successors) in 2-D: polytope 0 has n_source rows tangent to the unit circle, polytope 1 n_target rows tangent to
    the circle of radius 0.15 around (0.2, 0.1).  Under the contracting map theta+ = theta / 2 + (0.2, 0.1) of polytope 0 the pulled-back
    polygon C_01 is tangent to the circle of radius 0.3 around the origin, inside polytope 0: every one of its rows cuts, and child k of the
    difference carries polytope 0's rows, k earlier cutting rows and the reversed row: up to n_source + n_target rows, past the limit of 256,
    though every child is a polygon of far fewer sides.  Polytope 1 is sent far away.  The angles are regular with a seeded jitter of a
    fifth of a step, so no edge is short."""
    rng = numpy.random.default_rng(seed)
    polys = []
    for count, r, c in ((n_source, 1.0, numpy.zeros(2)), (n_target, 0.15, numpy.array([0.2, 0.1]))):
        ang = (numpy.arange(count) + 0.5 + rng.uniform(-0.2, 0.2, count)) * 2.0 * numpy.pi / count
        N = numpy.column_stack([numpy.cos(ang), numpy.sin(ang)])
        polys.append(numpy.column_stack([N @ c + r, N]))
    Phi = numpy.stack([0.5 * numpy.eye(2), numpy.eye(2)])
    phi = numpy.array([[0.2, 0.1], [50.0, 50.0]])
    return polys, Phi, phi, [[1], []]
