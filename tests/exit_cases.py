"""The inputs the exit-set tests share: the hand cases, worked out in the docstrings, and the seeded synthetic sets.  No
device and no package code: numpy only."""
import numpy

KINDS = ('contraction', 'rotation', 'rank_deficient', 'zero', 'identity')


def box_rows(lo, hi):
    """unit rows [o | n] of the box lo <= theta <= hi: the upper bounds, then the lower ones"""
    lo, hi = numpy.asarray(lo, dtype=float), numpy.asarray(hi, dtype=float)
    n = len(lo)
    return numpy.vstack([numpy.column_stack([hi, numpy.eye(n)]), numpy.column_stack([-lo, -numpy.eye(n)])])


def csr(polys):
    return numpy.concatenate([[0], numpy.cumsum([len(p) for p in polys])]).astype(numpy.int64), numpy.vstack(polys)


def intervals(pieces):
    """[(source, lo, hi)] of 1-D pieces given as (source, rows)"""
    out = []
    for src, rows in pieces:
        up, dn = rows[rows[:, 1] > 0], rows[rows[:, 1] < 0]
        out.append((int(src), float(numpy.max(-dn[:, 0] / -dn[:, 1])), float(numpy.min(up[:, 0] / up[:, 1]))))
    return out


def one_d_loop(a_plant):
    """min u^2, |u| <= 1, |2 theta + u| <= 0.5, |theta| <= 10 has the regions L = [-3/4, -1/4] (u = -1/2 - 2 theta), M = [-1/4, 1/4]
    (u = 0) and U = [1/4, 3/4] (u = 1/2 - 2 theta).  Under the plant theta+ = a theta + u:

      a = 2 (the model)  M: theta+ = 2 theta in [-1/2, 1/2], L: theta+ = -1/2, U: theta+ = 1/2: nothing leaves.
      a = 4 (mismatched) M: theta+ = 4 theta leaves [-3/4, 3/4] exactly on [-1/4, -3/16] and [3/16, 1/4], two pieces of length 1/16;
                         L: theta+ = 2 theta - 1/2 in [-2, -1] and U: theta+ = 2 theta + 1/2 in [1, 2] leave whole.  Exit volume 1.125 of 1.5.

    Returns (polys, Phi, phi, successors) in the order L, M, U; the successors by hand: a = 2: L -> L, M -> L, M, U, U -> U; a = 4:
    M -> L, M, U (4 theta in [-3/4, -1/4] on [-3/16, -1/16] and so on), L and U have none."""
    polys = [box_rows([-0.75], [-0.25]), box_rows([-0.25], [0.25]), box_rows([0.25], [0.75])]
    Phi = numpy.array([[[a_plant - 2.0]], [[float(a_plant)]], [[a_plant - 2.0]]])
    phi = numpy.array([[-0.5], [0.0], [0.5]])
    successors = [[0], [0, 1, 2], [2]] if a_plant == 2 else [[], [0, 1, 2], []]
    return polys, Phi, phi, successors


def grid_shift(shift=0.5):
    """The 3 x 3 unit cells of [0, 3]^2, cell 3 r + c = [c, c + 1] x [r, r + 1], all with theta+ = theta + (shift, 0): the images leave
    through the side x = 3 only.  A cell of the columns 0 and 1 lands in itself and its right neighbour and loses nothing of positive
    radius; a cell of column 2 keeps [2, 3 - shift] and leaves on [3 - shift, 3] x [r, r + 1]: one piece of area shift per row."""
    polys = [box_rows([c, r], [c + 1, r + 1]) for r in range(3) for c in range(3)]
    Phi = numpy.tile(numpy.eye(2), (9, 1, 1))
    phi = numpy.tile(numpy.array([shift, 0.0]), (9, 1))
    successors = [[3 * r + c] + ([3 * r + c + 1] if c < 2 else []) for r in range(3) for c in range(3)]
    return polys, Phi, phi, successors


def constant_rows():
    """Two squares A = [0, 1]^2 and B = [2, 3] x [0, 1] with the map (x, y) -> (x + 2, 1/2) on A and (x, y) -> (x, -1/2) on B.  Pulled back
    through A's map, B's rows in y are constant with beta = 1/2 >= 0 (dropped), its rows in x give 0 <= x <= 1: C_AB = R_A up to the
    dropped rows and A has no piece.  Through B's map every target's row -y <= 0 is constant with beta = -1/2 < -tol: C_BA and C_BB are
    empty, the piece stays and B leaves whole, whatever successors are passed."""
    polys = [box_rows([0, 0], [1, 1]), box_rows([2, 0], [3, 1])]
    Phi = numpy.tile(numpy.array([[1.0, 0.0], [0.0, 0.0]]), (2, 1, 1))
    phi = numpy.array([[2.0, 0.5], [0.0, -0.5]])
    return polys, Phi, phi, [[1], [0, 1]]


def _map(kind, n, act, rng):
    if kind == 'contraction':
        return 0.5 * numpy.eye(n) + 0.1 * rng.normal(size=(n, n)), rng.uniform(-0.3, 0.3, n)
    if kind == 'rotation':
        q, r = numpy.linalg.qr(rng.normal(size=(n, n)))
        return q * numpy.sign(numpy.diag(r)), numpy.zeros(n)
    if kind == 'rank_deficient':      # a zero row: the target rows along it are constant
        P = 0.5 * rng.normal(size=(n, n))
        P[int(rng.integers(0, act))] = 0.0
        return P, rng.uniform(-0.6, 0.6, n)
    if kind == 'zero':
        return numpy.zeros((n, n)), rng.uniform(-0.6, 0.6, n)
    # Phi = I with a shift: without one C_ii repeats the rows of R_i, every reversed row gives a candidate of radius exactly 0, and a
    # radius within 1e-7 of tol is a knife decision by definition
    shift = numpy.zeros(n)
    shift[:act] = rng.uniform(-0.2, 0.2, act)
    return numpy.eye(n), shift


def synthetic_set(n, seed, k, act=3, size=(0.25, 0.45)):
    """k bounded polytopes in [-1, 1]^n: a box around a centre that varies in the first ``act`` coordinates, cut by one to three random
    rows; the maps go round KINDS.  Bounded, so no radius run is unbounded."""
    rng = numpy.random.default_rng(seed)
    act = min(n, act)
    polys, Phi, phi = [], [], []
    for q in range(k):
        c, s = numpy.zeros(n), numpy.ones(n)
        c[:act], s[:act] = rng.uniform(-0.5, 0.5, act), rng.uniform(size[0], size[1], act)
        m = int(rng.integers(1, 4))
        N = rng.normal(size=(m, n))
        N /= numpy.linalg.norm(N, axis=1, keepdims=True)
        polys.append(numpy.vstack([box_rows(c - s, c + s), numpy.column_stack([N @ c + rng.uniform(0.1, 0.3, m), N])]))
        P, p = _map(KINDS[q % len(KINDS)], n, act, rng)
        Phi.append(P)
        phi.append(p)
    return polys, numpy.asarray(Phi), numpy.asarray(phi)


def tangent_pair(seed=14, n=16, rows=256):
    """Two polytopes of ``rows`` rows tangent to balls of radius 0.2 around c_0 and c_1 (an item of the pair holds 2 x rows rows: above
    48 KB of LDS at n = 16).  Polytope 0 is contracted by 0.05 onto c_1: its image lies within 0.05 x its width of c_1, deep inside
    polytope 1, so C_01 covers it, no row cuts and no piece is left.  Polytope 1 is sent far away and has no successor: it leaves whole.
    A piece may not exceed 256 rows, so a polytope of 256 rows admits no child at all: these two outcomes are the ones that exist."""
    rng = numpy.random.default_rng(seed)
    c = numpy.zeros((2, n))
    c[:, :2] = rng.uniform(-0.5, 0.5, (2, 2))
    polys = []
    for q in range(2):
        N = rng.normal(size=(rows, n))
        N /= numpy.linalg.norm(N, axis=1, keepdims=True)
        polys.append(numpy.column_stack([N @ c[q] + 0.2, N]))
    Phi = numpy.stack([0.05 * numpy.eye(n), numpy.eye(n)])
    phi = numpy.stack([c[1] - 0.05 * c[0], numpy.full(n, 50.0)])
    return polys, Phi, phi, [[1], []]


# (n_theta, seed, polytopes, varying coordinates, half-widths); the seeds were chosen on the CPU so that the reference reports no knife
# region (tests/test_exit_sets_cpu.py checks the first), the sizes so that the reference takes seconds: an image meets few polytopes
SETS = [(2, 21, 12, 2, (0.25, 0.45)), (3, 23, 24, 3, (0.12, 0.25)), (5, 23, 40, 5, (0.1, 0.18))]
