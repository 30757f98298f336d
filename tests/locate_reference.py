"""Point location and facet centres without the device kernels: the contract of include/mpcombi.h (mpc_locator_query,
mpc_facet_centres) restated in numpy, and generators of synthetic inputs whose answers are exact.

Membership:  strict all(E theta - f < tol), inclusive all(E theta <= f + tol); a region without rows contains no point (the rule of
loc_scan_lane / k_locate_few, unlike numpy.all([])); without overlap the first containing region wins, with overlap the containing
region of lowest objective 1/2 x'Qx + theta'H'x + c'x at x = A theta + b, ties to the later one; no region: -1 and x all NaN; a NaN
component of theta: -1.

Two precisions.
  exact  data on a dyadic lattice (multiples of 2^-12, |value| <= 2^8, tol 0 or 2^-10): every product and partial sum of a row test
         and of x = A theta + b then needs at most 12 + 12 + 8 + 8 + log2(17) < 46 bits, so float64 forms them without rounding, in
         any order and with or without fma.  The objective is a product of three such factors and needs more: exact_bits() bounds the
         width from the data, and the generators of overlap cases keep laws, Q, c, H and theta coarse enough for 53 bits.
  wide   random float64 data evaluated in numpy.longdouble; points whose answer the rounding of a float64 fma chain could change are
         left out (see locate_wide).
"""
import itertools

import numpy

LATTICE = 2.0 ** -12
TOL = 2.0 ** -10
U = 2.0 ** -53


# ---- the scan ---------------------------------------------------------------------------------------------------------------------
def _inside(rows, theta, tol, inclusive):
    """[m] bool: theta inside every row of `rows` ([k, n_t+1] = [f | E], k >= 1)"""
    v = theta @ rows[:, 1:].T
    if inclusive:
        return numpy.all(v <= rows[:, 0] + tol, axis=1)
    return numpy.all(v - rows[:, 0] < tol, axis=1)


def _objective(law, theta, Q, c, H):
    x = law[:, 0] + theta @ law[:, 1:].T
    g = numpy.zeros_like(x)
    if c is not None:
        g = g + c
    if H is not None:
        g = g + theta @ H.T
    if Q is not None:
        g = g + 0.5 * (x @ Q.T)
    return numpy.sum(g * x, axis=1)


def _cast(dtype, *arrays):
    return [None if a is None else numpy.asarray(a, dtype=dtype) for a in arrays]


def locate(row_off, ef, xlaw, theta, tol, overlapping=False, inclusive=False, Q=None, c=None, H=None, dtype=numpy.float64):
    """(region [m], x [m, n_x]) by the contract, evaluated in `dtype`"""
    ef, xlaw, theta, Q, c, H = _cast(dtype, ef, xlaw, theta, Q, c, H)
    n_x, n_t = xlaw.shape[1], xlaw.shape[2] - 1
    theta = theta.reshape(-1, n_t)
    if Q is not None:
        Q = Q.reshape(n_x, n_x)
    if c is not None:
        c = c.reshape(n_x)
    if H is not None:
        H = H.reshape(n_x, n_t)
    m = len(theta)
    found = numpy.full(m, -1, dtype=numpy.int64)
    best = numpy.full(m, numpy.inf, dtype=dtype)
    tol = dtype(tol)
    for r in range(len(row_off) - 1):
        rows = ef[row_off[r]:row_off[r + 1]]
        if len(rows) == 0:
            continue
        inside = _inside(rows, theta, tol, inclusive)
        if not overlapping:
            found[inside & (found < 0)] = r
            continue
        obj = _objective(xlaw[r], theta, Q, c, H)
        take = inside & (obj <= best)
        best[take] = obj[take]
        found[take] = r
    return found, evaluate(xlaw, theta, found)


def evaluate(xlaw, theta, region):
    """x = A theta + b of the region of every point, NaN where there is none (in the dtype of xlaw)"""
    n_x = xlaw.shape[1]
    x = numpy.full((len(theta), n_x), numpy.nan, dtype=xlaw.dtype)
    for r in numpy.unique(region[region >= 0]):
        sel = region == r
        x[sel] = xlaw[r][:, 0] + theta[sel] @ xlaw[r][:, 1:].T
    return x


def locate_wide(row_off, ef, xlaw, theta, tol, overlapping=False, inclusive=False, Q=None, c=None, H=None):
    """The contract in numpy.longdouble for float64 data: (region, x, keep [m] bool, x_bound [m, n_x]).

    keep is False for a point whose answer a float64 evaluation may change:
      * some row of some region has |(E theta - f) - tol| <= (n_t + 2) u (|f| + |E||theta|), u = 2^-53.  The strict test forms
        fma(E_t, theta_t, .) from -f, n_t roundings, |error| <= n_t u (|f| + |E||theta|) to first order; the inclusive test forms the
        product from 0 (n_t roundings) and rounds f + tol once.  The two spare u cover that, the second-order terms and the
        reference's own 2^-64 arithmetic.
      * with overlap, the two lowest objectives of containing regions are closer than the sum of their bounds
        (3 n_t + 2 n_x + 4) u sum_a G_a X_a with X = |b| + |A||theta| >= |x| and G = |c| + |H||theta| + 1/2 |Q| X >= |g|:
        x_a carries (n_t + 1) u X_a, g_a the chain over H (n_t), the inner product with Q (n_x) of x_j (n_t + 1 each) and one more
        fma, together (2 n_t + n_x + 2) u G_a, and the final sum over a another n_x u, all relative to sum G X; one u is spare.
    x_bound = (n_t + 1) u (|b| + |A||theta|) per component, the bound of k_evaluate's fma chain."""
    ld = numpy.longdouble
    efl, xl, th, Ql, cl, Hl = _cast(ld, ef, xlaw, theta, Q, c, H)
    n_x, n_t = xl.shape[1], xl.shape[2] - 1
    th = th.reshape(-1, n_t)
    region, x = locate(row_off, ef, xlaw, theta, tol, overlapping, inclusive, Q, c, H, dtype=ld)
    m = len(th)
    keep = numpy.ones(m, dtype=bool)
    ath = numpy.abs(th)
    objs, bounds = [], []
    for r in range(len(row_off) - 1):
        rows = efl[row_off[r]:row_off[r + 1]]
        if len(rows) == 0:
            continue
        v = th @ rows[:, 1:].T - rows[:, 0]
        mag = numpy.abs(rows[:, 0]) + ath @ numpy.abs(rows[:, 1:]).T
        keep &= ~numpy.any(numpy.abs(v - ld(tol)) <= (n_t + 2) * U * mag, axis=1)
        if overlapping:
            inside = _inside(rows, th, ld(tol), inclusive)
            X = numpy.abs(xl[r][:, 0]) + ath @ numpy.abs(xl[r][:, 1:]).T
            G = numpy.zeros_like(X)
            if cl is not None:
                G = G + numpy.abs(cl.reshape(n_x))
            if Hl is not None:
                G = G + ath @ numpy.abs(Hl.reshape(n_x, n_t)).T
            if Ql is not None:
                G = G + 0.5 * (X @ numpy.abs(Ql.reshape(n_x, n_x)).T)
            obj = _objective(xl[r], th, None if Ql is None else Ql.reshape(n_x, n_x), None if cl is None else cl.reshape(n_x),
                             None if Hl is None else Hl.reshape(n_x, n_t))
            objs.append(numpy.where(inside, obj, numpy.inf))
            bounds.append((3 * n_t + 2 * n_x + 4) * U * numpy.sum(G * X, axis=1))
    if overlapping and len(objs) >= 2:
        objs, bounds = numpy.array(objs), numpy.array(bounds)
        order = numpy.argsort(objs, axis=0)[:2]
        lo = numpy.take_along_axis(objs, order, axis=0)
        bd = numpy.take_along_axis(bounds, order, axis=0)
        both = numpy.isfinite(lo[1])
        gap = numpy.where(both, lo[1], 0.0) - numpy.where(both, lo[0], 0.0)
        keep &= ~(both & (gap <= bd[0] + bd[1]))
    x_bound = numpy.zeros((m, n_x))
    for r in numpy.unique(region[region >= 0]):
        sel = region == r
        x_bound[sel] = ((n_t + 1) * U * (numpy.abs(xl[r][:, 0]) + ath[sel] @ numpy.abs(xl[r][:, 1:]).T)).astype(float)
    return region, x, keep, x_bound


# ---- exactness of lattice data ----------------------------------------------------------------------------------------------------
def _unit(a):
    """(e, M): every entry of a is an integer multiple of 2^e (the largest such e, at most 0) and |a| <= M"""
    a = numpy.asarray(a, dtype=float).ravel()
    a = a[a != 0]
    if a.size == 0:
        return 0, 0.0
    for e in range(0, -64, -1):
        s = a * 2.0 ** -e
        if numpy.all(s == numpy.rint(s)):
            return e, float(numpy.max(numpy.abs(a)))
    raise ValueError('not on a dyadic lattice of 2^-63')


def _bits(e, M):
    return 0 if M == 0 else int(numpy.ceil(numpy.log2(M * 2.0 ** -e + 1)))


def exact_bits(ef, xlaw, theta, tol=0.0, Q=None, c=None, H=None):
    """(row, x, objective): bits that hold every partial sum of the row tests, of x = A theta + b and of the objective of these data.
    A sum of terms that are multiples of 2^e and bounded in total by M is a multiple of 2^e below M whatever the order, so it is a
    float64 when log2(M / 2^e) <= 53."""
    ef, xlaw, theta = numpy.asarray(ef, float), numpy.asarray(xlaw, float), numpy.asarray(theta, float)
    theta = theta[numpy.all(numpy.isfinite(theta), axis=-1)] if theta.size else theta
    n_t, n_x = xlaw.shape[2] - 1, xlaw.shape[1]
    et, Mt = _unit(theta)
    ee, Me = _unit(ef[:, 1:]) if len(ef) else (0, 0.0)
    ef_, Mf = _unit(numpy.r_[ef[:, 0], tol]) if len(ef) else (0, 0.0)
    row = _bits(min(ee + et, ef_), Mf + abs(tol) + n_t * Me * Mt)
    ea, Ma = _unit(xlaw[:, :, 1:]) if len(xlaw) else (0, 0.0)
    eb, Mb = _unit(xlaw[:, :, 0]) if len(xlaw) else (0, 0.0)
    ex, Mx = min(ea + et, eb), Mb + n_t * Ma * Mt
    eg, Mg = 0, 0.0
    if c is not None:
        eg, Mg = _unit(c)
    if H is not None:
        eh, Mh = _unit(H)
        eg, Mg = min(eg, eh + et), Mg + n_t * Mh * Mt
    if Q is not None:
        eq, Mq = _unit(Q)
        eg, Mg = min(eg, eq + ex - 1), Mg + 0.5 * n_x * Mq * Mx
    return row, _bits(ex, Mx), _bits(eg + ex, n_x * Mg * Mx)


def lattice(rng, shape, lo, hi, step=LATTICE):
    """uniform multiples of `step` in [lo, hi]"""
    return rng.integers(int(round(lo / step)), int(round(hi / step)) + 1, size=shape).astype(float) * step


# ---- builders of stacked regions -------------------------------------------------------------------------------------------------
def stack(regions, n_t):
    """regions: list of [k, n_t+1] row arrays (k may be 0) -> (row_off, ef)"""
    off = numpy.zeros(len(regions) + 1, dtype=numpy.int64)
    for i, r in enumerate(regions):
        off[i + 1] = off[i] + len(r)
    ef = numpy.vstack([numpy.asarray(r, float).reshape(-1, n_t + 1) for r in regions] + [numpy.zeros((0, n_t + 1))])
    return off, ef


def box_rows(lo, hi):
    """the 2 n_t rows [f | E] of {lo <= theta <= hi}: per axis the upper row, then the lower"""
    lo, hi = numpy.asarray(lo, float), numpy.asarray(hi, float)
    n = len(lo)
    rows = numpy.zeros((2 * n, n + 1))
    for a in range(n):
        rows[2 * a, 0], rows[2 * a, 1 + a] = hi[a], 1.0
        rows[2 * a + 1, 0], rows[2 * a + 1, 1 + a] = -lo[a], -1.0
    return rows


def padded(rows, k):
    """`rows` repeated cyclically to k rows: the same set of points"""
    rows = numpy.asarray(rows, float)
    return rows[numpy.arange(k) % len(rows)]


def lattice_laws(rng, R, n_x, n_t, step=LATTICE, bound=4.0):
    return lattice(rng, (R, n_x, n_t + 1), -bound, bound, step)


def random_polytopes(rng, n, m, R):
    """R random polytopes of m rows around random centres, every other one close to its predecessor (so that regions overlap), some
    with rows scaled by 1e3 and a duplicate row -- the mix of _random_polytopes in test_gpu_search_tree.py.  Returns (regions, centres)."""
    regs, centres = [], []
    for r in range(R):
        E = rng.normal(size=(m, n))
        c = rng.normal(size=n) * (10.0 if r % 3 == 0 else 1.0)
        if r % 2 == 1:
            c = centres[-1] + 0.02 * rng.normal(size=n)
        f = E @ c + rng.uniform(0.1, 1.0, size=m)
        if r % 4 == 1:
            E[::2] *= 1e3
            f[::2] *= 1e3
        if r % 5 == 2:
            E[1], f[1] = E[0], f[0]
        regs.append(numpy.c_[f, E])
        centres.append(c)
    return regs, numpy.array(centres)


def lattice_case(seed, n_t, n_x, coarse):
    """overlapping lattice boxes with a few oblique rows; `coarse`: laws, Q, c, H and theta on the coarse lattice of the overlap cases"""
    rng = numpy.random.default_rng(seed)
    regs, boxes = [], []
    for r in range(9):
        lo = lattice(rng, n_t, -3, -1, 0.25)
        size = lattice(rng, n_t, 2, 4, 0.25)
        rows = box_rows(lo, lo + size)
        extra = numpy.c_[lattice(rng, (2, 1), 4, 8, 0.25), lattice(rng, (2, n_t), -1, 1, 0.25)]
        regs.append(numpy.vstack([rows, extra]) if r % 2 else rows)
        boxes.append((lo, size))
    regs.insert(3, numpy.zeros((0, n_t + 1)))
    row_off, ef = stack(regs, n_t)
    step = 0.25 if coarse else LATTICE
    xlaw = lattice_laws(rng, len(regs), n_x, n_t, step, 2.0 if coarse else 4.0)
    xlaw[5] = xlaw[4]
    Q = lattice(rng, (n_x, n_x), -2, 2, 0.25)
    Q = Q + Q.T
    c, H = lattice(rng, n_x, -2, 2, 0.25), lattice(rng, (n_x, n_t), -2, 2, 0.25)
    fine = 0.0625 if coarse else LATTICE
    pick = [boxes[i] for i in rng.integers(0, 9, size=40)]
    theta = numpy.vstack([numpy.array([lo + lattice(rng, n_t, 0, 1, 0.25) * size for lo, size in pick[:20]]),       # facets included
                          numpy.array([lo + lattice(rng, n_t, 0, 2, fine) for lo, size in pick[20:]]),
                          lattice(rng, (20, n_t), -4, 4, fine), lattice(rng, (20, n_t), -4, 4, 0.25)])
    return row_off, ef, xlaw, Q, c, H, theta


WIDE_CASES = {   # (n_t, rows per region, regions): seed
    (3, 8, 40): 11,
    (8, 24, 20): 12,
    (16, 40, 12): 13,
}
WIDE_POINTS, WIDE_NX, WIDE_TOL = 2000, 3, 1e-5


def wide_case(shape):
    """The committed wide case of one shape: dict of row_off, ef, xlaw, Q, c, H, theta (2,000 points: near the centres, near the
    facets and far away)."""
    n, m, R = shape
    rng = numpy.random.default_rng(WIDE_CASES[shape])
    regs, centres = random_polytopes(rng, n, m, R)
    row_off, ef = stack(regs, n)
    xlaw = rng.normal(size=(R, WIDE_NX, n + 1))
    L = rng.normal(size=(WIDE_NX, WIDE_NX))
    quarter = WIDE_POINTS // 4
    pick = rng.integers(0, R, size=2 * quarter)
    pts = [centres[pick[:quarter]] + 0.02 * rng.normal(size=(quarter, n)),
           centres[pick[quarter:]] + 0.3 * rng.normal(size=(quarter, n)) / numpy.sqrt(n)]
    # on a row of a region, pushed +-{0.5, 2} tol along its normal
    rr = rng.integers(0, len(ef), size=quarter)
    base = centres[numpy.searchsorted(row_off, rr, side='right') - 1]
    E, f = ef[rr, 1:], ef[rr, 0]
    nn = numpy.sum(E * E, axis=1)
    k = rng.choice([-2.0, -0.5, 0.5, 2.0], size=quarter)
    pts.append(base - ((numpy.sum(E * base, axis=1) - f - k * WIDE_TOL) / nn)[:, None] * E)
    pts.append(rng.normal(size=(WIDE_POINTS - 3 * quarter, n)) * 5.0)
    return {'row_off': row_off, 'ef': ef, 'xlaw': xlaw, 'Q': L @ L.T + numpy.eye(WIDE_NX), 'c': rng.normal(size=WIDE_NX),
            'H': rng.normal(size=(WIDE_NX, n)), 'theta': numpy.vstack(pts), 'tol': WIDE_TOL}


# ---- thermometer grids: synthetic adjacency for the walk ---------------------------------------------------------------------------
KIND_LAMBDA, KIND_INACTIVE, KIND_OMEGA, KIND_UNKNOWN = 0, 1, 2, 3


class Grid:
    """An axis-aligned grid of boxes in n_t dimensions with the adjacency data of mpc_locator_set_adjacency.

    cuts: {axis: increasing lattice positions, k + 1 of them for k cells}; every other axis is only boxed by [-outer, outer].  The
    outer box is the parameter set.  Cell (i_a) has the active set  union_a {base_a .. base_a + i_a - 1}  (a thermometer code per axis);
    its upper row on axis a is the row of inactive constraint base_a + i_a (kind 1: behind it the cell with that id added, i_a + 1),
    its lower row the multiplier row of base_a + i_a - 1 (kind 0: behind it the cell without it, i_a - 1); on the outer box both are
    rows of the parameter set (kind 2).  Rows of a cell: per axis the upper one, then the lower one."""

    def __init__(self, n_t, cuts, bases, n_c, mask_words, outer=4.0):
        self.n_t, self.n_c, self.mask_words, self.outer = n_t, n_c, mask_words, outer
        self.axes = sorted(cuts)
        self.cuts = {a: numpy.asarray(cuts[a], float) for a in self.axes}
        self.bases = dict(bases)
        self.shape = tuple(len(self.cuts[a]) - 1 for a in self.axes)
        used = [self.bases[a] + j for a, k in zip(self.axes, self.shape) for j in range(k - 1)]
        assert len(set(used)) == len(used) and min(used) >= 0 and max(used) < n_c <= 64 * mask_words

    def all_cells(self):
        return list(itertools.product(*[range(k) for k in self.shape]))

    def shuffled(self, seed):
        cells = self.all_cells()
        order = numpy.random.default_rng(seed).permutation(len(cells))
        return [cells[i] for i in order]

    def active_set(self, cell):
        return [self.bases[a] + j for a, i in zip(self.axes, cell) for j in range(i)]

    def mask(self, cell):
        w = [0] * self.mask_words
        for i in self.active_set(cell):
            w[i >> 6] |= 1 << (i & 63)
        return w

    def cell_rows(self, cell):
        """(rows [2 n_t, n_t+1], info [2 n_t]) of one cell"""
        lo, hi = numpy.full(self.n_t, -self.outer), numpy.full(self.n_t, self.outer)
        info = numpy.full(2 * self.n_t, KIND_OMEGA << 16, dtype=numpy.int32)
        for a, i, k in zip(self.axes, cell, self.shape):
            lo[a], hi[a] = self.cuts[a][i], self.cuts[a][i + 1]
            if i < k - 1:
                info[2 * a] = KIND_INACTIVE << 16 | (self.bases[a] + i)
            if i > 0:
                info[2 * a + 1] = KIND_LAMBDA << 16 | (self.bases[a] + i - 1)
        return box_rows(lo, hi), info

    def build(self, cells, unknown=()):
        """Stacked arrays of the listed cells, in list order: dict of row_off, ef, row_info, masks (uint64 [R, words]), cells.
        unknown: cells whose rows are all of kind 3."""
        regs, infos, masks = [], [], []
        for cell in cells:
            rows, info = self.cell_rows(cell)
            if cell in unknown:
                info = numpy.full(len(info), KIND_UNKNOWN << 16, dtype=numpy.int32)
            regs.append(rows)
            infos.append(info)
            masks.append(self.mask(cell))
        row_off, ef = stack(regs, self.n_t)
        return {'row_off': row_off, 'ef': ef, 'row_info': numpy.concatenate(infos).astype(numpy.int32),
                'masks': numpy.array(masks, dtype=numpy.uint64).reshape(len(cells), self.mask_words), 'cells': list(cells)}

    def centre(self, cell, rng=None):
        """a lattice point well inside the cell (other axes: 0, or random inside the outer box with rng)"""
        p = numpy.zeros(self.n_t) if rng is None else lattice(rng, self.n_t, -self.outer + 1, self.outer - 1)
        for a, i in zip(self.axes, cell):
            p[a] = 0.5 * (self.cuts[a][i] + self.cuts[a][i + 1])
        return p

    def corner_points(self, offsets, rng=None):
        """every interior corner of the grid (one interior cut per cut axis) displaced by every combination of `offsets` per axis"""
        pts = []
        for corner in itertools.product(*[self.cuts[a][1:-1] for a in self.axes]):
            base = numpy.zeros(self.n_t) if rng is None else lattice(rng, self.n_t, -self.outer + 1, self.outer - 1)
            for d in itertools.product(offsets, repeat=len(self.axes)):
                p = base.copy()
                for a, c0, da in zip(self.axes, corner, d):
                    p[a] = c0 + da
                pts.append(p)
        return numpy.array(pts)

    def facet_points(self, offsets, rng=None):
        """cell centres moved to every cut of the cell's own axes (outer box included), displaced by `offsets` along that axis"""
        pts = []
        for cell in self.all_cells():
            for a, i in zip(self.axes, cell):
                for cut in (self.cuts[a][i], self.cuts[a][i + 1]):
                    for d in offsets:
                        p = self.centre(cell, rng)
                        p[a] = cut + d
                        pts.append(p)
        return numpy.array(pts)


GRIDS = {
    '2d': lambda: Grid(2, {0: numpy.arange(13) * 0.5 - 3.0, 1: numpy.arange(13) * 0.5 - 3.0}, {0: 58, 1: 100}, 128, 2),
    '3d': lambda: Grid(5, {0: numpy.arange(6) - 2.5, 1: numpy.arange(5) - 2.0, 2: numpy.arange(4) * 2.0 - 3.0}, {0: 61, 1: 0, 2: 126},
                           128, 2),
    '9d': lambda: Grid(9, {2: numpy.arange(7) - 3.0, 8: numpy.arange(7) - 3.0}, {2: 125, 8: 189}, 256, 4),
    '16d': lambda: Grid(16, {3: numpy.arange(7) - 3.0, 15: numpy.arange(7) - 3.0}, {3: 130, 15: 250}, 256, 4),
}


def walk_offsets(tol=TOL):
    return [s * k * tol for k in (0.5, 1.0, 2.0) for s in (-1.0, 1.0)]


# ---- facet centres -----------------------------------------------------------------------------------------------------------------
LP_OPTIMAL, LP_INFEASIBLE, LP_UNBOUNDED = 0, 1, 2
LP_TOL = 1e-9   # the relative LP tolerance of tests/test_gpu_theta_kernels.py


def facet_centre(rows, q):
    """(status, centre, radius) of facet q of {E theta <= f}, rows = [f | E]:  max r  s.t.  E_j theta + |E_j| r <= f_j (j != q),
    E_q theta = f_q, r >= 0, by scipy's HiGHS.  Centre and radius are 0 unless optimal."""
    from scipy.optimize import linprog
    rows = numpy.asarray(rows, float)
    f, E = rows[:, 0], rows[:, 1:]
    n = E.shape[1]
    others = numpy.arange(len(rows)) != q
    A_ub = numpy.c_[E[others], numpy.linalg.norm(E[others], axis=1)]
    kw = dict(A_ub=A_ub if others.any() else None, b_ub=f[others] if others.any() else None, A_eq=numpy.c_[E[q:q + 1], 0.0], b_eq=f[q:q + 1],
              bounds=[(None, None)] * n + [(0, None)], method='highs')
    cost = numpy.r_[numpy.zeros(n), -1.0]
    res = linprog(cost, **kw)
    if res.status == 4:   # "unbounded or infeasible" out of the presolve: ask again without it
        res = linprog(cost, options={'presolve': False}, **kw)
    status = {0: LP_OPTIMAL, 2: LP_INFEASIBLE, 3: LP_UNBOUNDED}[res.status]
    if status != LP_OPTIMAL:
        return status, numpy.zeros(n), 0.0
    return status, res.x[:n].copy(), float(res.x[n])


def facet_centres(row_off, ef):
    """(status [rows], centre [rows, n_t], radius [rows]) of every facet of the stacked polytopes, one LP each"""
    n_t = ef.shape[1] - 1
    st, ce, ra = numpy.zeros(len(ef), dtype=numpy.int32), numpy.zeros((len(ef), n_t)), numpy.zeros(len(ef))
    for r in range(len(row_off) - 1):
        rows = ef[row_off[r]:row_off[r + 1]]
        for q in range(len(rows)):
            st[row_off[r] + q], ce[row_off[r] + q], ra[row_off[r] + q] = facet_centre(rows, q)
    return st, ce, ra


def certificate_violation(rows, q, centre, radius):
    """How far (centre, radius) is from a feasible point of the LP of facet q, in units of the per-row scale
    1 + |f_j| + |E_j| |centre|_1:  max over rows of the residual / scale (<= LP_TOL for a certificate)."""
    rows = numpy.asarray(rows, float)
    f, E = rows[:, 0], rows[:, 1:]
    nrm = numpy.linalg.norm(E, axis=1)
    scale = 1.0 + numpy.abs(f) + nrm * numpy.sum(numpy.abs(centre))
    res = E @ centre + nrm * radius - f
    res[q] = abs(E[q] @ centre - f[q])
    return float(numpy.max(res / scale))


def tangent_polytope(rng, n, m, radius=1.0):
    """m rows tangent to the sphere of `radius` about a random centre: every row is a facet (its touching point is inside all others)"""
    E = rng.normal(size=(m, n))
    E /= numpy.linalg.norm(E, axis=1, keepdims=True)
    E *= rng.uniform(0.5, 2.0, size=(m, 1))
    c = rng.normal(size=n)
    return numpy.c_[E @ c + radius * numpy.linalg.norm(E, axis=1), E]


FACET_SHAPES = [(3, 63, 2), (3, 64, 3), (2, 127, 4), (3, 128, 5), (16, 64, 6)]   # (n_t, rows, seed) of the tangent polytopes


def box_facet_radius(sides, a):
    """radius of the facet on axis a of a box with the given side lengths: half the shortest other side, and at most the box's own
    extent along a (the opposite row); in one dimension only the latter"""
    others = [s / 2.0 for b, s in enumerate(sides) if b != a]
    return min(others + [sides[a]])


def simplex_rows(n):
    """{x >= 0, sum x <= 1}: rows -x_i <= 0 (radius 1 / (n - 1 + sqrt n)), then sum x <= 1 (radius 1 / n)"""
    return numpy.vstack([numpy.c_[numpy.zeros(n), -numpy.eye(n)], numpy.r_[1.0, numpy.ones(n)][None]])


def simplex_radii(n):
    return numpy.r_[numpy.full(n, 1.0 / (n - 1 + numpy.sqrt(n))), 1.0 / n]
