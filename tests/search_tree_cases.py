"""The inputs of the search-tree soundness tests (test_search_tree_cpu.py, test_gpu_search_tree.py): hand-built solutions,
their plane lists and candidates, and the exact classification of each by the CPU reference (search_tree_reference.py), solved once and
cached.  numpy and scipy only: nothing here needs a device.

Every case is knife-free by the reference alone: no lo within 1e-9 of -band, no hi within 1e-9 of +band, for every band the tests use
(test_cases_are_knife_free), so a device tree has to equal the reference tree node for node.
"""
import functools

import numpy

import compare_cases
import search_tree_reference as ref
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.solution import Solution
from ppopt_amd.upop.linear_code_gen import plane_table

TOL = 1e-5
BAND = 16 * TOL


class _Prog:
    def __init__(self, n_x, n_t, rng, quadratic=True):
        self.c = rng.normal(size=(n_x, 1))
        self.H = rng.normal(size=(n_x, n_t))
        if quadratic:
            M = rng.normal(size=(n_x, n_x))
            self.Q = M @ M.T + numpy.eye(n_x)
        self.c_c = numpy.zeros((1, 1))
        self.c_t = numpy.zeros((n_t, 1))
        self.Q_t = numpy.zeros((n_t, n_t))
        self._nt = n_t

    def num_t(self):
        return self._nt

    def evaluate_objective(self, x, th):
        v = th.T @ self.H.T @ x + self.c.T @ x
        if hasattr(self, 'Q'):
            v = v + 0.5 * x.T @ self.Q @ x
        return float(v[0, 0])


def _region(E, f, rng, n_x=2):
    E = numpy.asarray(E, float)
    n_t = E.shape[1]
    return CriticalRegion(rng.normal(size=(n_x, n_t)), rng.normal(size=(n_x, 1)), numpy.zeros((0, n_t)), numpy.zeros((0, 1)), E,
                          numpy.asarray(f, float).reshape(-1, 1), [])


def _triangles(rng, scale=1.0, centre=(0.0, 0.0), row_scales=None):
    """the box [-1, 1]^2 (scaled, shifted) cut by its diagonals into four triangles"""
    cx, cy = centre
    tri = [([[0, 1], [1, -1], [-1, -1]], [1, 0, 0]), ([[1, 0], [-1, 1], [-1, -1]], [1, 0, 0]),
           ([[0, -1], [-1, 1], [1, 1]], [1, 0, 0]), ([[-1, 0], [1, -1], [1, 1]], [1, 0, 0])]
    regs = []
    for k, (E, f) in enumerate(tri):
        E = numpy.array(E, float)
        f = numpy.array(f, float) * scale + E @ numpy.array([cx, cy])
        if row_scales is not None:
            s = numpy.array(row_scales[k % len(row_scales)], float)
            E, f = E * s[:, None], f * s
        regs.append(_region(E, f, rng))
    return regs


def _random_polytopes(rng, n, m, R):
    """R random polytopes with m rows in n dimensions around random centres, some with scaled and duplicate rows"""
    regs = []
    for r in range(R):
        E = rng.normal(size=(m, n))
        c = rng.normal(size=n) * (10.0 if r % 3 == 0 else 1.0)
        f = E @ c + rng.uniform(0.1, 1.0, size=m)
        if r % 4 == 1:
            E[::2] *= 1e3
            f[::2] *= 1e3
        if r % 5 == 2:
            E[1], f[1] = E[0], f[0]
        regs.append(_region(E, f, rng))
    return regs


# ---- the families -------------------------------------------------------------------------------------------------------------------------
PARTITIONS = {(1, 4): 80, (2, 6): 81, (3, 5): 82, (5, 5): 83, (16, 3): 84}   # (n, depth): seed of compare_cases.bsp
OVERLAPPING = [(6, 24, 10), (3, 8, 12)]
PLANE_COUNTS = [64, 65, 256, 257]
DUMMY_OFFSET = 50.0


def _partition(n, depth, seed, stack=False):
    rng = numpy.random.default_rng(1000 + seed)
    regs = []
    for cell in compare_cases.bsp(n, depth, seed):
        E, f = cell[:, 1:], cell[:, 0]
        if stack:   # the stacking of Solution.compare: the rows twice, every other row of the second copy scaled by 1e3
            s = numpy.where(numpy.arange(len(f)) % 2 == 0, 1e3, 1.0)
            E, f = numpy.vstack([E, E * s[:, None]]), numpy.concatenate([f, f * s])
        regs.append(_region(E, f, rng))
    return Solution(_Prog(2, n, rng), regs, point_location_tolerance=TOL)


def _overlapping(n, m, R):
    rng = numpy.random.default_rng(n * 100 + m)
    return Solution(_Prog(2, n, rng), _random_polytopes(rng, n, m, R), is_overlapping=True, point_location_tolerance=TOL)


def _edges():
    """the four triangles with, among them: a region without rows, one with a zero row 0 <= 1 (dropped), one with a zero row 0 <= -1
    (empty), one empty by contradiction (x <= 0, -x <= -1)"""
    rng = numpy.random.default_rng(7)
    t = _triangles(rng)
    small = _triangles(rng, scale=0.5, centre=(3.0, 0.5))
    no_rows = _region(numpy.zeros((0, 2)), numpy.zeros(0), rng)
    zero_ok = _region(numpy.vstack([small[0].E, [[0.0, 0.0]]]), numpy.r_[small[0].f.ravel(), 1.0], rng)
    zero_empty = _region(numpy.vstack([small[1].E, [[0.0, 0.0]]]), numpy.r_[small[1].f.ravel(), -1.0], rng)
    contradiction = _region([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]], [0.0, -1.0, 1.0, 1.0], rng)
    return Solution(_Prog(2, 2, rng), [t[0], no_rows, t[1], zero_ok, t[2], zero_empty, contradiction, t[3]], point_location_tolerance=TOL)


EDGE_NO_ROWS, EDGE_ZERO_DROPPED, EDGE_EMPTY = 1, 3, (5, 6)


def _pyramids(n):
    """the 2n cells {+-x_i >= |x_k| for k != i, +-x_i <= 1} of the box: 1 + 2 (n - 1) rows each, 2 (n - 1) of them through the apex"""
    rng = numpy.random.default_rng(20 + n)
    regs = []
    for i in range(n):
        for s in (1.0, -1.0):
            E, f = [s * numpy.eye(n)[i]], [1.0]
            for k in range(n):
                if k != i:
                    for q in (1.0, -1.0):
                        E.append(q * numpy.eye(n)[k] - s * numpy.eye(n)[i])
                        f.append(0.0)
            regs.append(_region(numpy.array(E), f, rng))
    return Solution(_Prog(2, n, rng), regs, point_location_tolerance=TOL)


FAN_THIN = (2, 6, 7)


def _fan():
    """twelve wedges around the origin in [-1, 1]^2; three of them open by 1e-4 rad, so their inverse basis reaches 1e4"""
    rng = numpy.random.default_rng(31)
    width = numpy.full(12, (2 * numpy.pi - 3e-4) / 9)
    width[list(FAN_THIN)] = 1e-4
    edge = 0.1 + numpy.concatenate([[0.0], numpy.cumsum(width)])
    box = compare_cases.box_rows(2)
    regs = []
    for k in range(12):
        a, b = edge[k], edge[k + 1]
        E = numpy.vstack([[[numpy.sin(a), -numpy.cos(a)], [-numpy.sin(b), numpy.cos(b)]], box[:, 1:]])
        regs.append(_region(E, numpy.r_[0.0, 0.0, box[:, 0]], rng))
    return Solution(_Prog(2, 2, rng), regs, point_location_tolerance=TOL)


_MAKERS = {f'part_{n}_{d}': functools.partial(_partition, n, d, seed) for (n, d), seed in PARTITIONS.items()}
_MAKERS.update({f'over_{n}_{m}': functools.partial(_overlapping, n, m, R) for n, m, R in OVERLAPPING})
_MAKERS.update({f'planes_{c}': functools.partial(_partition, 3, 5, PARTITIONS[3, 5]) for c in PLANE_COUNTS})
_MAKERS.update({'edges': _edges, 'pyramids_3': functools.partial(_pyramids, 3), 'pyramids_4': functools.partial(_pyramids, 4),
                'copies': functools.partial(_partition, 2, 4, 85, True), 'fan': _fan})
NAMES = sorted(_MAKERS)
DEGENERATE = ('pyramids_3', 'pyramids_4', 'copies', 'fan')
# builder arguments, run on two partitions: (leaf_size, max_depth, band, candidates from plane_table?)
ARG_CASES = ('part_2_6', 'part_3_5')
BANDS = (0.0, BAND, 0.1)
ARGS = [(leaf, depth, band, own) for leaf in (1, 3) for depth in (2, 48) for band in BANDS for own in (True, False)]


class Case:
    """One solution with the plane list and the candidates its trees are built from.  band: the default band of the case."""

    def __init__(self, name):
        self.name = name
        self.sol = _MAKERS[name]()
        self.ef, self.row_off, self.xlaw = self.sol._stacked()
        self.tol, self.band = TOL, BAND
        planes, start, plane_of, _ = plane_table(self.sol.critical_regions, self.sol.theta_dim())
        self.own_planes = planes
        self.n_dummy = 0
        if name.startswith('planes_'):   # dummy planes first: every region on their "-" side, so their key equals the node's size
            self.n_dummy = int(name.split('_')[1]) - len(planes)
            nrm = numpy.random.default_rng(9).normal(size=(220, planes.shape[1] - 1))[:self.n_dummy]
            nrm /= numpy.linalg.norm(nrm, axis=1, keepdims=True)
            self.planes = numpy.vstack([numpy.column_stack([nrm, numpy.full(self.n_dummy, DUMMY_OFFSET)]), planes])
            self.cand = None
        else:
            self.planes = planes
            self.cand = (start, plane_of)

    @property
    def n_regions(self):
        return len(self.row_off) - 1


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def _own_classification(key):
    """the LPs of a solution against its own plane table, once per solution (the plane-count cases share the (3, 5) partition's)"""
    c = case(key)
    return ref.classify(c.ef, c.row_off, c.own_planes, c.tol, c.band)


@functools.lru_cache(maxsize=None)
def classification(name, band=None):
    """the exact classification of a case at a band (default: the case's own)"""
    c = case(name)
    band = c.band if band is None else band
    own = _own_classification('part_3_5' if c.n_dummy else name)
    if not c.n_dummy:
        return ref.reband(own, band)
    # a dummy plane: s = n.theta - 50 over P^ inside the box |theta_i| <= 1 + tol, so the interval bound decides its side by a margin of
    # 48; no dummy plane may become a node's plane (their lo / hi are bounds, not LP values), which the tests assert of the reference tree
    R, D = c.n_regions, c.n_dummy
    reach = numpy.abs(c.planes[:D, :-1]).sum(axis=1) * (1 + c.tol)
    lo = numpy.hstack([numpy.tile(-reach - DUMMY_OFFSET, (R, 1)), own[2]])
    hi = numpy.hstack([numpy.tile(reach - DUMMY_OFFSET, (R, 1)), own[3]])
    allow = numpy.concatenate([numpy.zeros((R, D, 2)), own[4]], axis=1)
    out = ref.Classification((lo >= -band, hi <= band, lo, hi, allow))
    out.xopt = numpy.concatenate([numpy.full((R, D, 2, own.xopt.shape[3]), numpy.nan), own.xopt], axis=1)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, leaf_size=1, max_depth=48, band=None, own=True):
    """the reference tree of a case; own: candidates from the plane table (where the case has them), else every plane"""
    c = case(name)
    band = c.band if band is None else band
    cand = c.cand if own and c.cand is not None else (None, None)
    return ref.build(c.ef, c.row_off, c.planes, cand[0], cand[1], c.tol, band, leaf_size, max_depth, cls=classification(name, band))


def check(name, arrays, leaf_size=1, max_depth=48, band=None, own=True):
    """ref.check_tree of any builder's arrays for a case and its builder arguments"""
    c = case(name)
    band = c.band if band is None else band
    return ref.check_tree(arrays, c.ef, c.row_off, c.tol, band, classification(name, band), max_depth, leaf_size,
                          c.cand if own and c.cand is not None else None)


def witnesses(name, arrays, band=None):
    c = case(name)
    return ref.witness_points(arrays, c.ef, c.row_off, c.tol, classification(name, band))
