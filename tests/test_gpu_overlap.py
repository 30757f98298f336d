"""Solution.remove_overlaps on the device: partition_by_value against the independent CPU reference on the hand-built
cases and on random polytopes in a box up to n_theta = 16 and 200 rows, properties that need no reference (ownership by sampling,
volumes, determinism), solved programs (an mpLP and a two-parameter mpMILP), the refusals of the two library calls and one raw item
of the row loop with a result derived by hand."""
import warnings

import numpy
import pytest

import overlap_reference as ref
from ppopt_amd import _lib
from ppopt_amd.geometry import Polytope, polytope_volumes
from ppopt_amd.overlap import VERDICTS, partition_by_value
from test_overlap_cpu import CASES, box_rows, check_by_sampling, cut_lines

pytestmark = pytest.mark.gpu

TOL = 1e-8


def _csr(polys):
    return numpy.concatenate([[0], numpy.cumsum([len(p) for p in polys])]).astype(numpy.int64), numpy.vstack(polys)


def _canonical(rows):
    rows = numpy.asarray(rows, dtype=float)
    return rows[numpy.lexsort(numpy.round(rows, 6).T[::-1])]


def _device(polys, g, h):
    off, ef = _csr(polys)
    return partition_by_value(off, ef, g, h, polys[0].shape[1] - 1)


def _same_as_reference(polys, part, want):
    """1 (exempt, nothing compared) when the reference met an LP value within its KNIFE of a threshold; else verdicts equal, r, d_min,
    d_max within 1e-9 (1 + |value|), the same sources and every piece's rows within 1e-9 after a canonical sort"""
    if want['knife']:
        return 1
    got = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(part.pairs['i'], part.pairs['j']))}
    for pair, verdict in want['verdicts'].items():       # a pair the device's boxes do not even meet is DISJOINT
        k = got.get(pair)
        assert (VERDICTS[part.pairs['verdict'][k]] if k is not None else 'DISJOINT') == verdict, pair
        if k is None:
            continue
        for name, w in zip(('radius', 'd_min', 'd_max'), want['values'][pair]):
            v = part.pairs[name][k]
            if numpy.isnan(w) or numpy.isinf(w):
                assert (numpy.isnan(v) and numpy.isnan(w)) or v == w, (pair, name, v, w)
            else:
                assert abs(v - w) <= 1e-9 * (1.0 + abs(w)), (pair, name, v, w)
    for pair, k in got.items():
        assert pair in want['verdicts'] or VERDICTS[part.pairs['verdict'][k]] == 'DISJOINT', pair
    assert part.sources.tolist() == want['sources'].tolist()
    assert part.vanished == want['vanished']
    for k, (p, q, whole) in enumerate(zip(part.pieces, want['pieces'], want['whole'])):
        assert (p is None) == whole, k
        rows = polys[part.sources[k]] if p is None else p
        assert rows.shape == q.shape, k
        numpy.testing.assert_allclose(_canonical(rows), _canonical(q), rtol=0, atol=1e-9)
    return 0


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_the_reference_on_the_hand_built_cases(name):
    """exempt cases: 0 of 9 (asserted)"""
    polys, g, h = CASES[name]
    part = _device(polys, g, h)
    assert _same_as_reference(polys, part, ref.partition_reference(polys, g, h)) == 0
    st = part.stats
    assert st['regions_before'] == len(polys) and st['regions_after'] == len(part.pieces) and st['lps'] > 0
    assert sum(part.verdict_counts.values()) == st['candidate_pairs']


# ---- random polytopes in a box ---------------------------------------------------------------------------------------------------
def random_case(n, seed, k, balls=(), act=3, size=(0.25, 0.45)):
    """k polytopes in the box [-1, 1]^n (a small box around a centre that varies in the first ``act`` coordinates, with half-widths in
    ``size`` there and the whole box elsewhere, cut by one to three random rows), regions of ``balls`` rows tangent to a ball of radius 0.2, and
    the box itself, last, as the most expensive region; random affine values"""
    rng = numpy.random.default_rng(seed)
    act = min(n, act)
    polys = []
    for _ in range(k):
        c, s = numpy.zeros(n), numpy.ones(n)
        c[:act], s[:act] = rng.uniform(-0.5, 0.5, act), rng.uniform(size[0], size[1], act)
        m = int(rng.integers(1, 4))
        N = rng.normal(size=(m, n))
        N /= numpy.linalg.norm(N, axis=1, keepdims=True)
        polys.append(numpy.vstack([box_rows(c - s, c + s), numpy.column_stack([N @ c + rng.uniform(0.1, 0.3, m), N])]))
    for m in balls:
        c = numpy.zeros(n)
        c[:act] = rng.uniform(-0.5, 0.5, act)
        N = rng.normal(size=(m, n))
        N /= numpy.linalg.norm(N, axis=1, keepdims=True)
        polys.append(numpy.column_stack([N @ c + 0.2, N]))
    polys.append(box_rows(-numpy.ones(n), numpy.ones(n)))
    g = numpy.vstack([rng.normal(size=(len(polys) - 1, n)), numpy.zeros((1, n))])
    h = numpy.append(rng.normal(size=len(polys) - 1), 100.0)
    return polys, g, h


# (n_theta, seed, polytopes, ball regions): 6 to 12 polytopes besides the box; the ball regions of 65 and 200 rows make the lane loop over
# rows span several 64-row chunks, give cutters of more than 64 rows and items whose P and C together exceed 256 rows
RANDOM = [(1, 1, 6, ()), (2, 2, 8, ()), (2, 3, 4, (65, 200), 2, (0.15, 0.3)), (3, 4, 6, (), 3, (0.2, 0.35)), (3, 5, 4, (65, 200), 3, (0.15, 0.3)),
          (5, 6, 6, (), 2, (0.12, 0.25)), (16, 7, 6, (), 1, (0.04, 0.1))]
_RUNS = {}


def _run(case):
    if case not in _RUNS:
        polys, g, h = random_case(*case)
        _RUNS[case] = (polys, g, h, _device(polys, g, h))
    return _RUNS[case]


@pytest.mark.parametrize('case', RANDOM, ids=[f'n{c[0]}_s{c[1]}' for c in RANDOM])
def test_random_cases_against_the_reference(case):
    """exempt cases: 0 of 7 with these seeds (the reference alone, run on the CPU).  The cap of 2 % of 7 cases is below one case, so
    none may be exempt."""
    polys, g, h, part = _run(case)
    assert _same_as_reference(polys, part, ref.partition_reference(polys, g, h)) == 0


@pytest.mark.parametrize('case', [RANDOM[2], RANDOM[4]], ids=['n2', 'n3'])
def test_the_ball_regions_reach_the_wide_paths(case):
    """the 200-row region G is the last cutter of the box: some item of that round holds more than 256 rows (piece, cutter and cut row
    together), and some piece of the result carries the reversed row k >= 64 of G, so a bit of the mask words 1 to 3 was set and read"""
    polys, g, h, part = _run(case)
    assert [len(p) for p in polys[4:6]] == [65, 200]
    G = polys[5]
    assert part.stats['rounds'] >= 2 and part.stats['wide'] == 0
    if case[0] == 3:      # in 2-D no piece that meets G has more than 56 rows
        assert part.stats['max_item_rows'] > 256
    high = {k for p in part.pieces if p is not None for k in range(64, 200) if numpy.any(numpy.all(p == -G[k], axis=1))}
    assert {k >> 6 for k in high} == {1, 2, 3}, 'no piece was cut off by a row of G in each of the mask words 1 to 3'


@pytest.mark.parametrize('case', RANDOM, ids=[f'n{c[0]}_s{c[1]}' for c in RANDOM])
def test_ownership_by_sampling(case):
    polys, g, h, part = _run(case)
    n = case[0]
    pieces = [polys[s] if p is None else p for p, s in zip(part.pieces, part.sources)]
    pts = numpy.random.default_rng(100 + case[1]).uniform(-1.0, 1.0, size=(20000, n))
    kept = check_by_sampling(polys, g, h, pieces, part.sources, pts, clear=1e-6, lines=cut_lines(polys, g, h))
    assert kept > 15000


@pytest.mark.parametrize('case', [c for c in RANDOM if c[0] <= 5], ids=[f'n{c[0]}_s{c[1]}' for c in RANDOM if c[0] <= 5])
def test_the_pieces_fill_the_box(case):
    """the box is a region, so the union of the pieces is the box: the volumes add up to 2^n within 1e-9.  (n_theta = 16 is left to the
    sampling test: a piece there keeps most of the 65,536 vertices of the box.)"""
    polys, g, h, part = _run(case)
    pieces = [polys[s] if p is None else p for p, s in zip(part.pieces, part.sources)]
    vol = polytope_volumes([Polytope(p[:, 1:], p[:, 0]) for p in pieces])
    assert numpy.all(vol.status == _lib.VOL_OK), numpy.bincount(vol.status)
    total = float(vol.volume.sum())
    print(f'volume {total!r} of {2.0 ** case[0]}')
    assert abs(total - 2.0 ** case[0]) <= 1e-9 * 2.0 ** case[0]


def test_two_runs_give_identical_results():
    polys, g, h, a = _run(RANDOM[4])
    b = _device(polys, g, h)
    assert a.sources.tolist() == b.sources.tolist() and a.vanished == b.vanished and a.verdict_counts == b.verdict_counts
    for name in ('i', 'j', 'verdict', 'radius', 'd_min', 'd_max'):
        numpy.testing.assert_array_equal(a.pairs[name], b.pairs[name])
    for p, q in zip(a.pieces, b.pieces):
        assert (p is None) == (q is None)
        if p is not None:
            numpy.testing.assert_array_equal(p, q)
    for k in ('rounds', 'work_items', 'lps', 'pivots', 'wide', 'candidate_pairs'):
        assert a.stats[k] == b.stats[k], k


def degenerate_mplp():
    """min x1 + x2  s.t.  x1 + x2 >= theta1 + 2, 0 <= x1 <= theta2 + 2, 0 <= x2 <= 3 - theta2 on the box |theta| <= 1: no bilinear term,
    and the objective is parallel to the first row, so every vertex of that row is optimal.  A solved mpLP whose optimal bases are
    unique is a partition already (all its pairs come out DISJOINT); this one has four regions with the value theta1 + 2 that overlap
    pairwise, and all four rows of its parameter box survive the presolve, so coverage_volume has a volume to divide by."""
    from ppopt_amd import MPLP_Program
    A = numpy.array([[-1.0, -1.0], [-1.0, 0.0], [0.0, -1.0], [1.0, 0.0], [0.0, 1.0]])
    F = numpy.array([[-1.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    b = numpy.array([[-2.0], [0.0], [0.0], [2.0], [3.0]])
    return MPLP_Program(A, b, numpy.ones((2, 1)), numpy.zeros((2, 2)), numpy.vstack([numpy.eye(2), -numpy.eye(2)]), numpy.ones((4, 1)), F)


# ---- solved programs -----------------------------------------------------------------------------------------------------------------
_SOLVED = {}


def _solved(name):
    if name not in _SOLVED:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if name == 'mplp':
                from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
                prog = degenerate_mplp()
                sol = solve_mpqp(prog, mpqp_algorithm.combinatorial)
            else:
                from ppopt_amd.mp_solvers.solve_mpmiqp import solve_mpmiqp
                from test_gpu_mi import _load, build
                prog = build(_load('mpMILP_market_problem'))
                sol = solve_mpmiqp(prog, num_cores=1)
        _SOLVED[name] = (prog, sol, sol.remove_overlaps())
    return _SOLVED[name]


def _theta_points(prog, red, m, seed):
    """m points of the bounding box of the parameter set that lie at least 1e-4 from every row of every piece: the locator takes a
    point within point_location_tolerance = 1e-5 of a piece as inside, so closer to a boundary two pieces may claim it"""
    A_t, b_t = numpy.asarray(prog.A_t, dtype=float), numpy.asarray(prog.b_t, dtype=float).reshape(-1)
    box = ref.box_of(ref.Record(), ref.unit(A_t, b_t))
    rows = numpy.vstack([ref.unit(r.E, r.f) for r in red.critical_regions])
    # where the rows of the parameter set leave a coordinate open, the box of the pieces (a tenth wider) stands in
    each = [ref.box_of(ref.Record(), ref.unit(r.E, r.f)) for r in red.critical_regions]
    lo, hi = numpy.min([b[0] for b in each], axis=0), numpy.max([b[1] for b in each], axis=0)
    assert numpy.all(numpy.isfinite(lo)) and numpy.all(numpy.isfinite(hi))
    box = (numpy.where(numpy.isfinite(box[0]), box[0], lo - 0.1 * (hi - lo)), numpy.where(numpy.isfinite(box[1]), box[1], hi + 0.1 * (hi - lo)))
    rng = numpy.random.default_rng(seed)
    out = numpy.zeros((0, A_t.shape[1]))
    while len(out) < m:
        pts = rng.uniform(box[0], box[1], size=(2 * m, A_t.shape[1]))
        out = numpy.vstack([out, pts[numpy.all(numpy.abs(pts @ rows[:, 1:].T - rows[:, 0]) >= 1e-4, axis=1)]])
    return out[:m], box


def _objective(prog, x, th):
    return numpy.array([prog.evaluate_objective(x[k].reshape(-1, 1), th[k].reshape(-1, 1)) for k in range(len(th))])


@pytest.mark.parametrize('name', ['mplp', 'mpmilp'])
def test_solved_programs(name):
    prog, sol, red = _solved(name)
    assert sol.is_overlapping and len(sol) >= 2
    with pytest.raises(ValueError):
        sol.coverage_volume()
    assert not red.is_overlapping and red.overlap_info['source'] is sol and red.overlap_info['stats']['lps'] > 0
    assert [r.source for r in red.critical_regions] == red.overlap_info['sources'].tolist()
    counts, st = red.overlap_info['verdict_counts'], red.overlap_info['stats']
    print(f'{name}: verdicts {counts}, rounds {st["rounds"]}, work items {st["work_items"]}, LPs {st["lps"]}')
    assert st['candidate_pairs'] >= 1 and sum(counts.values()) == st['candidate_pairs']      # k_overlap_pairs ran
    assert sum(v for k, v in counts.items() if k != 'DISJOINT') >= 1 and st['rounds'] >= 1 and st['work_items'] >= 1
    th, box = _theta_points(prog, red, 10000, 5)
    x_s, reg_s = sol.evaluate_batch(th)
    x_r, reg_r = red.evaluate_batch(th)
    numpy.testing.assert_array_equal(reg_s >= 0, reg_r >= 0)
    numpy.testing.assert_array_equal(reg_r, red.get_region_batch(th))
    hit = reg_r >= 0
    assert hit.sum() > 100
    J_s, J_r = _objective(prog, x_s[hit], th[hit]), _objective(prog, x_r[hit], th[hit])
    print(f'{name}: {len(sol)} regions -> {len(red)} pieces, max |J_red - J_src| / (1 + |J|) = {numpy.max(numpy.abs(J_r - J_s) / (1 + numpy.abs(J_s))):.3e}')
    assert numpy.all(numpy.abs(J_r - J_s) <= 1e-9 * (1.0 + numpy.abs(J_s)))
    if name == 'mpmilp':
        det = prog.solve_theta_batch(th[hit])
        J_d = numpy.array([d.obj for d in det])
        assert numpy.all(numpy.abs(J_r - J_d) <= 1e-7 * (1.0 + numpy.abs(J_d)))
    cov = red.coverage_volume()
    assert cov.ok and cov.fraction <= 1.0 + 1e-9
    # the share of the parameter set the pieces cover, against the hit rate of the same points among those in the parameter set
    inside = numpy.all(th @ numpy.asarray(prog.A_t).T <= numpy.asarray(prog.b_t).reshape(1, -1), axis=1)
    rate, n_in = float(hit[inside].mean()), int(inside.sum())
    se = max(numpy.sqrt(max(cov.fraction * (1.0 - cov.fraction), 0.0) / n_in), 1.0 / n_in)
    print(f'{name}: coverage {cov.fraction:.6f}, hit rate {rate:.6f} of {n_in} points, 3 se = {3 * se:.6f}')
    assert abs(rate - cov.fraction) <= 3.0 * se
    tree = red.search_tree()
    numpy.testing.assert_array_equal(tree.locate_batch(th), reg_r)


def test_a_qp_solution_is_refused_with_the_quadratic_part_message():
    from ppopt_amd import MPQP_Program, problem_generator as pg
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    d = pg.transport_mpqp_data()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sol = solve_mpqp(MPQP_Program(d['A'], d['b'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], d['F']), mpqp_algorithm.combinatorial)
    with pytest.raises(ValueError, match='quadratic value functions is not convex and is out of scope'):
        sol.remove_overlaps()


# ---- the library's refusals ------------------------------------------------------------------------------------------------------------
def test_library_refusals():
    """MPC_ERR_INVALID (MpcError with the library's message) before any launch"""
    sq = box_rows([0, 0], [1, 1])
    off, ef = _csr([sq, sq + numpy.array([0.5, 0, 0])])
    xs = numpy.zeros((2, 2))
    pairs = lambda **kw: _lib.overlap_pairs(kw.get('off', off), kw.get('ef', ef), kw.get('xs', xs), kw.get('a', [0]), kw.get('b', [1]),
                                            kw.get('hc', [0]), kw.get('cut'), kw.get('tol', TOL))
    split = lambda **kw: _lib.overlap_split(kw.get('off', off), kw.get('ef', ef), kw.get('poff', off[:2]), kw.get('pef', ef[:4]), kw.get('p', [0]),
                                            kw.get('c', [1]), kw.get('hc', [0]), kw.get('cut'), kw.get('start'), kw.get('tol', TOL))
    assert pairs()[3].tolist() == [0] and split()[0].tolist() == [_lib.OVERLAP_MEETS]        # the good calls these are variations of
    nan = ef.copy()
    nan[1, 1] = numpy.nan
    long = numpy.vstack([sq] * 65)
    wide = numpy.hstack([numpy.ones((4, 1)), numpy.eye(17)[:4]])
    for call, kw, text in ((pairs, {'tol': -1.0}, 'tol'), (split, {'tol': -1.0}, 'tol'), (pairs, {'ef': nan}, 'finite'), (split, {'ef': nan}, 'finite'),
                           (split, {'pef': nan[:4]}, 'finite'), (pairs, {'b': [2]}, 'out of range'), (pairs, {'a': [-1]}, 'out of range'),
                           (split, {'p': [1]}, 'out of range'), (split, {'c': [2]}, 'out of range'),
                           (pairs, {'off': [0, 260], 'ef': long, 'xs': xs[:1], 'a': [], 'b': [], 'hc': []}, '1..256 rows'),
                           (split, {'poff': [0, 260], 'pef': long}, '1..256 rows'), (split, {'poff': [0, 0, 4], 'p': [1]}, '1..256 rows'),
                           (pairs, {'off': [0, 4], 'ef': wide, 'xs': numpy.zeros((1, 17)), 'a': [], 'b': [], 'hc': []}, 'n_t must lie in 1..16'),
                           (pairs, {'hc': [1], 'cut': [[0.0, 2.0, 0.0]]}, 'unit normals'), (pairs, {'xs': xs * numpy.inf}, 'finite')):
        with pytest.raises(_lib.MpcError, match=text):
            call(**kw)


def test_the_row_loop_with_rows_that_do_not_cut_between_rows_that_do():
    """One raw item of mpc_overlap_split, expected result derived by hand.  Piece [0, 1]^2 from (0.5, 0.5); cutter x <= 2, x <= 0.5, y <= 3,
    y <= 0.5, -x <= 0.25 and the cut row x + y <= 0.75.  Rows 1 and 3 cut, rows 0, 2 and 4 do not (the reversed row leaves the piece), so
    the slot a reversed row is written to falls behind the slot its row is read from; the cut row cuts last, in the triangle
    (0.25, 0.5), (0.5, 0.25), (0.5, 0.5).  Seven LPs: the intersection and six rows."""
    cutter = numpy.array([[2, 1, 0], [0.5, 1, 0], [3, 0, 1], [0.5, 0, 1], [0.25, -1, 0]], dtype=float)
    s = 1.0 / numpy.sqrt(2.0)
    flag, mask, stats = _lib.overlap_split([0, 5], cutter, [0, 4], box_rows([0, 0], [1, 1]), [0], [0], [1], [[0.75 * s, s, s]], [[0.5, 0.5]], TOL)
    assert mask[0].tolist() == [0b01010, 0, 0, 0]
    assert flag[0] == _lib.OVERLAP_MEETS | _lib.OVERLAP_CUT_ROW
    assert stats['items'] == stats['meets'] == 1
    assert stats['lps'] == 7
    assert stats['wide'] == 0
