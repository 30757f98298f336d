"""The overlap removal of DESIGN §3.19 on the host: the independent reference (overlap_reference.py) on hand-built cases with known
answers and on the 1-D mixed-integer goldens against the brute-force minimum, then the host pieces of ppopt_amd/overlap.py that need
no device: build_reduced_solution, get_region / evaluate on its result, and every refusal of remove_overlaps."""
import glob
import os

import numpy
import pytest

import overlap_reference as ref
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.solution import Solution
from test_mi_host import _ObjectiveOnly, unpack_regions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MI_FILES = sorted(glob.glob(os.path.join(GOLDEN, 'mi_*.npz')))


class ValueProg:
    """The little of a program that value_function and get_region read: objective c.x + theta^T H^T x + 1/2 x^T Q x.  With the default
    n_x = 1, c = 1, a region's law x = A theta + b is its value function."""

    def __init__(self, n_t, n_x=1, Q=None):
        self._nt = n_t
        self.c, self.H = numpy.ones((n_x, 1)), numpy.zeros((n_x, n_t))
        self.c_t, self.Q_t, self.c_c = numpy.zeros((n_t, 1)), numpy.zeros((n_t, n_t)), numpy.zeros((1, 1))
        if Q is not None:
            self.Q = numpy.asarray(Q, dtype=float)

    def num_t(self):
        return self._nt

    def evaluate_objective(self, x, th):
        x, th = numpy.asarray(x, dtype=float).reshape(-1, 1), numpy.asarray(th, dtype=float).reshape(-1, 1)
        v = th.T @ self.H.T @ x + self.c.T @ x
        if hasattr(self, 'Q'):
            v = v + 0.5 * x.T @ self.Q @ x
        return float(v[0, 0])


def box_rows(lo, hi):
    """unit rows [o | n] of the box lo <= theta <= hi"""
    lo, hi = numpy.asarray(lo, dtype=float), numpy.asarray(hi, dtype=float)
    n = len(lo)
    return numpy.vstack([numpy.column_stack([hi, numpy.eye(n)]), numpy.column_stack([-lo, -numpy.eye(n)])])


def value_solution(polys, g, h, overlapping=True):
    """a Solution over ValueProg whose region i is polys[i] with the value g_i.theta + h_i"""
    n_t = polys[0].shape[1] - 1
    regs = [CriticalRegion(numpy.asarray(g[i], dtype=float).reshape(1, n_t), numpy.array([[float(h[i])]]), numpy.zeros((0, n_t)),
                           numpy.zeros((0, 1)), p[:, 1:].copy(), p[:, :1].copy(), [i]) for i, p in enumerate(polys)]
    s = Solution(ValueProg(n_t), regs, is_overlapping=overlapping, point_location_tolerance=1e-9)
    s.is_complete = True
    return s


def interval(rows):
    """(lo, hi) of a 1-D piece"""
    up, dn = rows[rows[:, 1] > 0], rows[rows[:, 1] < 0]
    return float(numpy.max(dn[:, 0] / dn[:, 1])), float(numpy.min(up[:, 0] / up[:, 1]))


def area(rows, big=10.0):
    """area of a 2-D piece: the square [-big, big]^2 clipped by every row"""
    poly = [(-big, -big), (big, -big), (big, big), (-big, big)]
    for o, a, b in rows:
        out = []
        for k in range(len(poly)):
            p, q = poly[k], poly[(k + 1) % len(poly)]
            sp, sq = a * p[0] + b * p[1] - o, a * q[0] + b * q[1] - o
            if sp <= 0:
                out.append(p)
            if (sp < 0 < sq) or (sq < 0 < sp):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        poly = out
        if len(poly) < 3:
            return 0.0
    x, y = numpy.array(poly).T
    return 0.5 * abs(float(numpy.dot(x, numpy.roll(y, -1)) - numpy.dot(y, numpy.roll(x, -1))))


def triangle(p, q, r):
    """unit rows of the triangle p q r (counter-clockwise)"""
    rows = []
    for a, b in ((p, q), (q, r), (r, p)):
        a, b = numpy.asarray(a, dtype=float), numpy.asarray(b, dtype=float)
        nrm = numpy.array([b[1] - a[1], a[0] - b[0]])
        nrm /= numpy.linalg.norm(nrm)
        rows.append(numpy.append(nrm @ a, nrm))
    return numpy.asarray(rows)


# name: (polytopes, g, h)
CASES = {
    '1d_second_cheaper_on_overlap': ([box_rows([0], [2]), box_rows([1], [3])], [[1.0], [-1.0]], [0.0, 2.0]),
    '1d_values_cross_inside': ([box_rows([0], [2]), box_rows([1], [3])], [[1.0], [-1.0]], [0.0, 3.0]),
    '1d_inner_cheaper': ([box_rows([0], [3]), box_rows([1], [2])], [[0.0], [0.0]], [0.0, -1.0]),
    '2d_inner_square_cheaper': ([box_rows([0, 0], [2, 2]), box_rows([0.5, 0.5], [1.5, 1.5])], [[0.0, 0.0], [0.0, 0.0]], [0.0, -1.0]),
    '2d_cross_at_1_5': ([box_rows([0, 0], [2, 2]), box_rows([1, 0], [3, 2])], [[1.0, 0.0], [-1.0, 0.0]], [0.0, 3.0]),
    'equal_values': ([box_rows([0], [2]), box_rows([1], [3])], [[0.5], [0.5]], [1.0, 1.0]),
    'dominated_everywhere': ([box_rows([0], [3]), box_rows([1], [2])], [[0.0], [0.0]], [0.0, 1.0]),
    'three_triangles': ([triangle((0, 0), (2, 0), (1, 2)), triangle((1, 0), (3, 0), (2, 2)), triangle((0.5, 1), (1.5, -1), (2.5, 1))],
                        [[1.0, 0.0], [-1.0, 0.5], [0.0, 1.0]], [0.0, 2.0, 0.3]),
    'disjoint': ([box_rows([0, 0], [1, 1]), box_rows([2, 0], [3, 1]), box_rows([0, 2], [1, 3])], [[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]],
                 [0.0, 1.0, 2.0]),
}


def run_case(name):
    polys, g, h = CASES[name]
    return ref.partition_reference(polys, g, h)


def by_source(out):
    return {i: [p for p, s in zip(out['pieces'], out['sources']) if s == i] for i in range(int(max(out['sources'], default=-1)) + 1)}


def test_1d_second_cheaper_on_overlap():
    out = run_case('1d_second_cheaper_on_overlap')
    assert out['verdicts'] == {(0, 1): 'J_WINS'} and out['sources'].tolist() == [0, 1]
    numpy.testing.assert_allclose([interval(p) for p in out['pieces']], [(0, 1), (1, 3)], atol=1e-12)


def chain(pieces):
    """(lo, hi) of 1-D pieces that follow one another without a gap (pieces of one source are not merged back)"""
    iv = sorted(interval(p) for p in pieces)
    for a, b in zip(iv, iv[1:]):
        assert a[1] == pytest.approx(b[0], abs=1e-12)
    return iv[0][0], iv[-1][1]


def test_1d_values_cross_inside():
    out = run_case('1d_values_cross_inside')
    assert out['verdicts'] == {(0, 1): 'CROSSING'} and out['sources'].tolist() == [0, 0, 1, 1]
    numpy.testing.assert_allclose([chain(out['pieces'][:2]), chain(out['pieces'][2:])], [(0, 1.5), (1.5, 3)], atol=1e-12)
    r, d_min, d_max = out['values'][(0, 1)]
    numpy.testing.assert_allclose([r, d_min, d_max], [0.5, -0.5, 0.5], atol=1e-12)


def test_1d_inner_cheaper_gives_three_pieces():
    out = run_case('1d_inner_cheaper')
    assert out['verdicts'] == {(0, 1): 'J_WINS'} and out['sources'].tolist() == [0, 0, 1]
    assert sorted(interval(p) for p in out['pieces']) == pytest.approx([(0, 1), (1, 2), (2, 3)])
    assert out['whole'] == [False, False, True]


def test_2d_inner_square_cheaper():
    out = run_case('2d_inner_square_cheaper')
    assert out['sources'].tolist() == [0, 0, 0, 0, 1] and out['vanished'] == []
    assert sum(area(p) for p in out['pieces'][:4]) == pytest.approx(3.0, abs=1e-12)
    assert area(out['pieces'][4]) == pytest.approx(1.0, abs=1e-12)
    for a in range(4):       # the outer pieces share boundaries only
        for b in range(a + 1, 4):
            assert area(numpy.vstack([out['pieces'][a], out['pieces'][b]])) == pytest.approx(0.0, abs=1e-12)


def test_2d_values_cross_at_one_and_a_half():
    out = run_case('2d_cross_at_1_5')
    assert out['verdicts'] == {(0, 1): 'CROSSING'} and out['sources'].tolist() == [0, 0, 1, 1]
    for mine, (lo, hi) in ((out['pieces'][:2], (0.0, 1.5)), (out['pieces'][2:], (1.5, 3.0))):
        assert sum(area(p) for p in mine) == pytest.approx(3.0, abs=1e-12)
        boxes = [ref.box_of(ref.Record(), p) for p in mine]
        numpy.testing.assert_allclose([min(b[0][0] for b in boxes), max(b[1][0] for b in boxes)], [lo, hi], atol=1e-9)


def test_equal_values_the_lower_index_loses_the_overlap():
    out = run_case('equal_values')
    assert out['verdicts'] == {(0, 1): 'EQUAL'} and out['sources'].tolist() == [0, 1]
    numpy.testing.assert_allclose([interval(p) for p in out['pieces']], [(0, 1), (1, 3)], atol=1e-12)


def test_a_region_dominated_everywhere_vanishes():
    out = run_case('dominated_everywhere')
    assert out['verdicts'] == {(0, 1): 'I_WINS'} and out['sources'].tolist() == [0] and out['vanished'] == [1]
    assert out['whole'] == [True]


def contains(rows, pts, margin=0.0):
    return numpy.all(pts @ rows[:, 1:].T <= rows[:, 0] + margin, axis=1)


def check_by_sampling(polys, g, h, pieces, sources, pts, clear=1e-6, lines=()):
    """Of the points at least ``clear`` from every source row, piece row and line of ``lines``: exactly one piece contains a point that
    some source region contains, none otherwise, and the piece's source attains the minimum value over the containing sources within
    1e-9 (1 + |J|).  Returns the number of points checked."""
    g, h = numpy.asarray(g, dtype=float), numpy.asarray(h, dtype=float)
    every = numpy.vstack(list(polys) + list(pieces) + [numpy.asarray(c).reshape(-1, pts.shape[1] + 1) for c in lines])
    pts = pts[numpy.all(numpy.abs(pts @ every[:, 1:].T - every[:, 0]) >= clear, axis=1)]
    inside = numpy.array([contains(p, pts) for p in polys])                      # [R, m]
    J = g @ pts.T + h[:, None]
    best = numpy.where(inside, J, numpy.inf).min(axis=0)
    hits = numpy.array([contains(p, pts) for p in pieces]) if len(pieces) else numpy.zeros((0, len(pts)), dtype=bool)
    n_hit = hits.sum(axis=0)
    assert numpy.array_equal(n_hit, inside.any(axis=0).astype(int)), 'a covered point is not in exactly one piece (or an uncovered one is)'
    src = numpy.asarray(sources)[numpy.argmax(hits, axis=0)] if len(pieces) else numpy.zeros(len(pts), dtype=int)
    cov = n_hit == 1
    got = J[src[cov], numpy.flatnonzero(cov)]
    assert numpy.all(numpy.abs(got - best[cov]) <= 1e-9 * (1.0 + numpy.abs(best[cov])))
    return len(pts)


def cut_lines(polys, g, h):
    """the planes J_i = J_j of all pairs with different slopes, as unit rows"""
    g, h = numpy.asarray(g, dtype=float), numpy.asarray(h, dtype=float)
    out = []
    for i in range(len(polys)):
        for j in range(i + 1, len(polys)):
            d = g[i] - g[j]
            if numpy.linalg.norm(d) > 1e-12:
                out.append(numpy.append(h[i] - h[j], -d) / numpy.linalg.norm(d))
    return out


def test_three_mutually_overlapping_triangles_by_sampling():
    polys, g, h = CASES['three_triangles']
    out = ref.partition_reference(polys, g, h)
    assert set(out['verdicts']) == {(0, 1), (0, 2), (1, 2)} and 'DISJOINT' not in out['verdicts'].values()
    pts = numpy.random.default_rng(7).uniform([-0.5, -1.5], [3.5, 2.5], size=(20000, 2))
    assert check_by_sampling(polys, g, h, out['pieces'], out['sources'], pts, lines=cut_lines(polys, g, h)) > 19000


def test_disjoint_regions_come_back_unchanged():
    polys, g, h = CASES['disjoint']
    out = ref.partition_reference(polys, g, h)
    assert out['sources'].tolist() == [0, 1, 2] and out['whole'] == [True, True, True] and out['vanished'] == []
    assert all(v == 'DISJOINT' for v in out['verdicts'].values())
    for p, q in zip(out['pieces'], polys):
        numpy.testing.assert_array_equal(p, q)


REDUCIBLE = [p for p in MI_FILES if numpy.load(p)['proc_F'].shape[1] == 1 and 'proc_Q' not in numpy.load(p).files]


def test_some_goldens_are_reducible():
    assert len(REDUCIBLE) >= 1


@pytest.mark.parametrize('path', REDUCIBLE, ids=[os.path.basename(p)[3:-4] for p in REDUCIBLE])
def test_goldens_1d_the_piece_of_a_point_attains_the_brute_force_minimum(path):
    g = numpy.load(path)
    prog, regs = _ObjectiveOnly(g), unpack_regions(g, 'P_')
    src = Solution(prog, regs, is_overlapping=True)
    out = ref.reduce_reference(src)
    polys = [ref.unit(r.E, r.f) for r in regs]
    spans = numpy.array([interval(p) for p in polys])
    pts = numpy.random.default_rng(11).uniform(spans[:, 0].min() - 0.05, spans[:, 1].max() + 0.05, size=(1000, 1))
    n_in = 0
    for th in pts:
        J = [prog.evaluate_objective(r.evaluate(th.reshape(-1, 1)), th.reshape(-1, 1)) for r in regs]
        inside = [i for i, p in enumerate(polys) if contains(p, th[None])[0]]
        owners = [int(s) for p, s in zip(out['pieces'], out['sources']) if contains(p, th[None], 1e-12)[0]]
        if not inside:
            assert not owners
            continue
        n_in += 1
        assert owners, f'theta = {th[0]} lies in a region and in no piece'
        best = min(J[i] for i in inside)
        for s in owners:
            assert abs(J[s] - best) <= 1e-9, (th[0], s, J[s], best)
    assert n_in > 100


# ---- the host pieces of ppopt_amd/overlap.py ---------------------------------------------------------------------------------------
def _reduced(name):
    from ppopt_amd.overlap import build_reduced_solution
    polys, g, h = CASES[name]
    src = value_solution(polys, g, h)
    out = ref.partition_reference(polys, g, h)
    rows = [None if w else p for p, w in zip(out['pieces'], out['whole'])]
    return src, out, build_reduced_solution(src, out['sources'], rows, {'J_WINS': 1}, out['vanished'], {'rounds': 1})


def test_build_reduced_solution():
    from ppopt_amd.overlap import ReducedRegion, build_reduced_solution
    src, out, red = _reduced('1d_inner_cheaper')
    assert not red.is_overlapping and red.is_complete and red.program is src.program
    assert red.point_location_tolerance == src.point_location_tolerance
    assert [r.source for r in red.critical_regions] == [0, 0, 1] and all(isinstance(r, ReducedRegion) for r in red.critical_regions)
    info = red.overlap_info
    assert info['source'] is src and info['sources'].tolist() == [0, 0, 1] and info['vanished'] == [] and info['stats'] == {'rounds': 1}
    assert info['verdict_counts'] == {'J_WINS': 1}
    whole = red.critical_regions[2]
    numpy.testing.assert_array_equal(whole.E, src.critical_regions[1].E)
    numpy.testing.assert_array_equal(whole.f, src.critical_regions[1].f)
    assert whole.E is not src.critical_regions[1].E
    for r in red.critical_regions:
        s = src.critical_regions[r.source]
        numpy.testing.assert_array_equal(r.A, s.A)
        numpy.testing.assert_array_equal(r.b, s.b)
        assert r.active_set == s.active_set and r.f.shape == (r.E.shape[0], 1)
    assert src.overlap_info is None and Solution(None, []).overlap_info is None and len(src) == 2
    _, _, gone = _reduced('dominated_everywhere')
    assert gone.overlap_info['vanished'] == [1] and len(gone) == 1
    with pytest.raises(ValueError):
        build_reduced_solution(src, [1, 0], [None, None])
    with pytest.raises(ValueError):
        build_reduced_solution(src, [0, 2], [None, None])


def test_mixed_integer_fields_are_carried():
    from ppopt_amd.overlap import build_reduced_solution
    g = numpy.load(REDUCIBLE[0])
    regs = unpack_regions(g, 'P_')
    src = Solution(_ObjectiveOnly(g), regs, is_overlapping=True)
    red = build_reduced_solution(src, [0], [None])
    r = red.critical_regions[0]
    assert list(r.y_fixation) == list(regs[0].y_fixation) and list(r.y_indices) == list(regs[0].y_indices)
    assert list(r.x_indices) == list(regs[0].x_indices)
    numpy.testing.assert_array_equal(r.C, regs[0].C)


@pytest.mark.parametrize('name', ['1d_values_cross_inside', '2d_inner_square_cheaper', 'three_triangles'])
def test_get_region_and_evaluate_of_the_result_agree_with_the_source(name):
    src, out, red = _reduced(name)
    n_t = src.theta_dim()
    rng = numpy.random.default_rng(3)
    n_in = 0
    for th in rng.uniform(-0.5, 3.5, size=(400, n_t)):
        th = th.reshape(-1, 1)
        a, b = src.get_region(th), red.get_region(th)
        assert (a is None) == (b is None)
        if a is not None:
            n_in += 1
            assert src.program.evaluate_objective(red.evaluate(th), th) == pytest.approx(src.program.evaluate_objective(src.evaluate(th), th), abs=1e-9)
    assert n_in > 50


def test_remove_overlaps_refusals():
    """every ValueError comes before anything reaches the device (there is none here)"""
    polys, g, h = CASES['1d_values_cross_inside']
    good = value_solution(polys, g, h)
    with pytest.raises(ValueError, match='no regions'):
        Solution(ValueProg(1), [], is_overlapping=True).remove_overlaps()
    merged = value_solution(polys, g, h)
    merged.merge_info = {'source': good}
    with pytest.raises(ValueError, match='merged'):
        merged.remove_overlaps()
    wide = value_solution([box_rows([0] * 17, [1] * 17)], [[0.0] * 17], [0.0])
    with pytest.raises(ValueError, match='n_theta = 17'):
        wide.remove_overlaps()
    many = value_solution([numpy.vstack([box_rows([0], [1])] * 129)], [[0.0]], [0.0])
    with pytest.raises(ValueError, match='more than 256 rows'):
        many.remove_overlaps()
    for kw in ({'tol': float('nan')}, {'tol': float('inf')}, {'value_tol': float('nan')}, {'tol': -1.0}):
        with pytest.raises(ValueError, match='finite'):
            good.remove_overlaps(**kw)
    quad = value_solution(polys, [[1.0], [0.5]], h)      # 1/2 x^T Q x along x = A theta + b: quadratic parts 2 and 0.5
    quad.program = ValueProg(1, Q=[[2.0]])
    with pytest.raises(ValueError, match='quadratic value functions is not convex and is out of scope'):
        quad.remove_overlaps()
    assert good.overlap_info is None


def test_coverage_volume_still_refuses_sources():
    polys, g, h = CASES['1d_values_cross_inside']
    with pytest.raises(ValueError, match='overlapping'):
        value_solution(polys, g, h).coverage_volume()
