"""Solution.compare on the device (csrc/compare.hpp, ppopt_amd/compare.py) against the CPU reference of compare_reference.py,
the hand cases of compare_cases.py and sampled points."""
import functools
import warnings

import numpy
import pytest
from scipy.optimize import linprog

import compare_cases as cases
import compare_reference as ref
from ppopt_amd import MPQP_Program, Solution, _lib, compare as cmp, problem_generator as pg
from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
from ppopt_amd.region_merge import solution_rows

pytestmark = pytest.mark.gpu

TOL = 1e-8
KNIFE_SHARE = 0.02       # of a set's pairs


def _close(got, want):
    """within 1e-9 (1 + |value|); infinities exactly"""
    if numpy.isinf(want) or numpy.isinf(got):
        return got == want
    return abs(got - want) <= 1e-9 * (1.0 + abs(want))


def _unflagged(sol):
    """solve_mpqp flags every solution it returns as overlapping, as the reference does; the regions of a strictly convex mpQP do not
    overlap, and compare refuses by the flag: the same program and regions without it"""
    if not sol.is_overlapping:
        return sol
    assert numpy.linalg.eigvalsh(sol.program.Q).min() > 0
    plain = Solution(sol.program, sol.critical_regions, is_overlapping=False, point_location_tolerance=sol.point_location_tolerance)
    plain.is_complete = sol.is_complete
    return plain


def _solved(d):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        prog = MPQP_Program(d['A'], d['b'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], d['F'], equality_indices=d.get('equality_indices'))
        return _unflagged(solve_mpqp(prog, mpqp_algorithm.combinatorial))


@functools.lru_cache(maxsize=None)
def _one_d(c):
    return _solved(cases.one_d_program_data(c))


@functools.lru_cache(maxsize=None)
def _double_integrator(horizon):
    return _solved(pg.double_integrator_data(horizon=horizon))


def _tables(a, b, out_a, out_b):
    """(polys, laws, n_a) of two solutions in one table, assembled here from the regions: the rows out_a of a's laws against out_b of b's"""
    n_t = a.theta_dim()
    polys, laws = [], []
    for s, outs in ((a, out_a), (b, out_b)):
        off, rows, void = solution_rows(s.critical_regions, n_t, 'test')
        assert not void
        polys += numpy.split(rows, off[1:-1])
        for r in s.critical_regions:
            laws.append(numpy.hstack([numpy.asarray(r.b).reshape(-1, 1), numpy.asarray(r.A).reshape(-1, n_t)])[outs])
    return polys, numpy.asarray(laws), len(a.critical_regions)


def _witness_holds(polys, laws, i, j, row, witness, gap):
    """the witness lies in both polytopes within 1e-9, and |delta_row(witness)| from the two laws is the gap within 1e-9 (1 + gap)"""
    for p in (polys[i], polys[j]):
        assert numpy.all(p[:, 1:] @ witness <= p[:, 0] + 1e-9), (i, j)
    d = laws[i][row] - laws[j][row]
    assert abs(abs(d[0] + d[1:] @ witness) - gap) <= 1e-9 * (1.0 + gap), (i, j, row, d[0] + d[1:] @ witness, gap)


def _against_reference(polys, laws, res, max_knife=None):
    """every pair of res against the reference: the same pairs meet, radius, lo, hi and gap within 1e-9 (1 + |value|), infinities, rows and
    flags exactly, witnesses of unflagged meeting pairs; knife pairs are exempt.  Returns (the reference, knife pairs)."""
    pairs = list(zip(res['i'].tolist(), res['j'].tolist()))
    want = ref.gap_reference(polys, laws, pairs, TOL)
    knife = 0
    for k, pair in enumerate(pairs):
        w = want[pair]
        if w['knife']:
            knife += 1
            continue
        what = (pair, {key: res[key][k] for key in ('radius', 'gap', 'row', 'flag')}, w)
        assert _close(res['radius'][k], w['radius']), what
        assert int(res['flag'][k]) == w['flag'], what
        if not w['meets']:
            assert numpy.isnan(res['gap'][k]) and res['row'][k] == -1 and numpy.all(numpy.isnan(res['witness'][k])), what
            assert numpy.all(numpy.isnan(res['ranges'][k])), what
            continue
        assert _close(res['gap'][k], w['gap']), what
        if numpy.isinf(w['radius']):
            assert res['row'][k] == -1 and numpy.all(numpy.isnan(res['ranges'][k])), what
            continue
        for r in range(len(w['lo'])):
            assert _close(res['ranges'][k, r, 0], w['lo'][r]) and _close(res['ranges'][k, r, 1], w['hi'][r]), (what, r)
        per_row = numpy.maximum(-res['ranges'][k, :, 0], res['ranges'][k, :, 1])
        assert res['gap'][k] == per_row.max() and res['row'][k] == int(numpy.argmax(per_row)), what      # the lowest row that attains it
        if not w['flag']:
            _witness_holds(polys, laws, pair[0], pair[1], int(res['row'][k]), res['witness'][k], res['gap'][k])
    limit = int(KNIFE_SHARE * len(pairs)) if max_knife is None else max_knife
    assert knife <= limit, (knife, len(pairs))
    return want, knife


# ---- 1. hand cases -------------------------------------------------------------------------------------------------------------------------
def _by_interval(sol):
    """region indices (left, middle, right) of a solved 1-D program by their centres"""
    mids = []
    for r in sol.critical_regions:
        E, f = numpy.asarray(r.E).reshape(-1), numpy.asarray(r.f).reshape(-1)
        keep = E != 0.0
        b = f[keep] / E[keep]
        mids.append(0.5 * (b[E[keep] > 0].min() + b[E[keep] < 0].max()))
    return numpy.argsort(mids).tolist()


def test_one_d_program_by_hand():
    """compare_cases.one_d_by_hand and test_compare_cpu.test_reference_one_d_by_hand: the largest gap is 0.1, reached by an LP at
    theta = 0.3 on [.25, .3] and by the constant difference -0.1 on [.3, .75]; [.3, .8] of the c = 0.6 solution is covered to 0.9"""
    a, b = _one_d(0.5), _one_d(0.6)
    assert len(a) == len(b) == 3
    g = a.compare(b, ranges=True, coverage=True)
    assert _close(g.max_gap, 0.1) and g.row[g.argmax] == 0 and g.wide == 0
    assert len(g.unmatched_a) == 0 and len(g.unmatched_b) == 0 and not g.equal(0.05) and g.equal(0.1 + 1e-9)
    (la, ma, ra), (lb, mb, rb) = _by_interval(a), _by_interval(b)
    pair = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(g.i, g.j))}
    assert sorted(p for p, k in pair.items() if g.meets[k]) == sorted([(la, lb), (la, mb), (ma, mb), (ra, mb), (ra, rb)])
    lp, const, mid = pair[(ra, mb)], pair[(ra, rb)], pair[(ma, mb)]
    assert _close(g.radius[lp], 0.025) and _close(g.gap[lp], 0.1) and _close(g.witness[lp, 0], 0.3)
    assert _close(g.ranges[lp, 0, 0], -0.1) and _close(g.ranges[lp, 0, 1], 0.0)
    assert _close(g.radius[const], 0.225) and _close(g.gap[const], 0.1)
    assert _close(g.ranges[const, 0, 0], -0.1) and _close(g.ranges[const, 0, 1], -0.1)
    if numpy.array_equal(a.critical_regions[ra].A, b.critical_regions[rb].A):      # a constant row: the Chebyshev centre of [.3, .75]
        assert _close(g.witness[const, 0], 0.525)
    assert 0.3 - 1e-9 <= g.witness[const, 0] <= 0.75 + 1e-9
    assert g.gap[mid] == 0.0 and _close(g.radius[mid], 0.25)
    for side, (l, m, r), other in ((g.covered_a, (la, ma, ra), None), (g.covered_b, (lb, mb, rb), 0.9)):
        assert _close(side[m], 1.0) and _close(side[l], side[r]) and _close(side[r], 1.0 if other is None else other)
    numpy.testing.assert_allclose(g.gap_of_a[[la, ma, ra]], [0.1, 0.0, 0.1], rtol=0, atol=2e-10)


def test_hand_arrays_and_open_cases():
    """the hand-built arrays of the 1-D case (exact constant rows), and the open cases in 2-D"""
    pa, la = cases.one_d_by_hand(0.5)
    pb, lb = cases.one_d_by_hand(0.6)
    off, ef = cases.csr(pa + pb)
    laws = numpy.concatenate([la, lb])
    i, j = numpy.divmod(numpy.arange(9), 3)
    res = cmp.law_gap_pairs(off, ef, laws, i, j + 3, tol=TOL, ranges=True)
    _against_reference(pa + pb, laws, res, max_knife=0)
    k = 2 * 3 + 2
    assert _close(res['gap'][k], 0.1) and _close(res['witness'][k, 0], 0.525)                   # right against right: the centre of [.3, .75]
    assert _close(res['gap'][2 * 3 + 1], 0.1) and _close(res['witness'][2 * 3 + 1, 0], 0.3)     # right against middle: the LP's vertex
    assert res['stats'] == dict(res['stats'], pairs=9, meets=5, constant_rows=3, lps=9 + 2 * 2, wide=0)
    polys, laws, pairs = cases.open_quadrant()
    off, ef = cases.csr(polys)
    res = cmp.law_gap_pairs(off, ef, laws, [p for p, _ in pairs], [q for _, q in pairs], tol=TOL, ranges=True)
    _against_reference(polys, laws, res, max_knife=0)
    assert res['radius'][0] == numpy.inf and res['gap'][0] == numpy.inf and res['row'][0] == -1 and res['flag'][0] == 1
    assert numpy.all(numpy.isfinite(res['witness'][0])) and res['flag'][1] == 0 and _close(res['gap'][1], 3.0)
    assert res['stats']['lps'] == 2 + 2 and res['stats']['wide'] == 1 and res['stats']['meets'] == 1
    polys, laws, pairs = cases.open_half_strip()
    off, ef = cases.csr(polys)
    res = cmp.law_gap_pairs(off, ef, laws, [p for p, _ in pairs], [q for _, q in pairs], tol=TOL, ranges=True)
    _against_reference(polys, laws, res, max_knife=0)
    assert res['gap'][0] == numpy.inf and res['ranges'][0, 0, 1] == numpy.inf and _close(res['ranges'][0, 0, 0], 0.0) and res['flag'][0] == 1
    assert res['row'][0] == 0 and _close(res['radius'][0], 0.5)
    assert _close(res['gap'][1], 1.0) and res['flag'][1] == 0 and _close(res['ranges'][1, 0, 0], 0.0) and _close(res['ranges'][1, 0, 1], 1.0)
    assert res['stats']['wide'] == 1 and res['stats']['meets'] == 2


# ---- 2. to 4. synthetic sets -------------------------------------------------------------------------------------------------------------
def _run_set(case):
    """candidates by cross_box_pairs over the boxes of _lib.merge_regions, then the pair stage: (polys, laws, n_a, res)"""
    polys, laws, n_a = cases.table(case)
    off, ef = cases.csr(polys)
    xs, box, status, _ = _lib.merge_regions(off, ef)
    assert numpy.all(status == 0)
    pa, pb = cmp.cross_box_pairs(box[:n_a], status[:n_a] == 0, box[n_a:], status[n_a:] == 0, TOL)
    assert numpy.all(numpy.diff(pa * len(polys) + pb) > 0)           # ascending by (i, j)
    res = cmp.law_gap_pairs(off, ef, laws, pa, pb + n_a, tol=TOL, xs=xs, ranges=True)
    return polys, laws, n_a, res


@functools.lru_cache(maxsize=None)
def _all_radii(n):
    """the reference radius of every pair (A cell, B cell) of synthetic(n)"""
    case = cases.synthetic(n)
    return numpy.array([[ref.radius(numpy.vstack([p, q])) for q in case['polys_b']] for p in case['polys_a']])


@pytest.mark.parametrize('n', sorted(cases.SHAPES))
def test_synthetic_sets_against_the_reference(n):
    case = cases.synthetic(n)
    polys, laws, n_a, res = _run_set(case)
    # the candidates are a superset of the reference's meeting pairs, and the shapes are the ones that were checked
    radii = _all_radii(n)
    meeting = {(int(i), int(j) + n_a) for i, j in zip(*numpy.nonzero(radii > TOL))}
    assert len(meeting) == cases.SHAPES[n][3] and not numpy.any(numpy.abs(radii - TOL) <= ref.KNIFE)
    cand = set(zip(res['i'].tolist(), res['j'].tolist()))
    assert meeting <= cand
    want, knife = _against_reference(polys, laws, res)
    assert knife == 0
    assert {p for p, w in want.items() if w['meets']} == meeting == {p for k, p in enumerate(zip(res['i'].tolist(), res['j'].tolist()))
                                                                     if not numpy.isnan(res['gap'][k])}
    # 4. constant rows: a copied law gives gap 0.0 exactly and runs no LP; the counters count exactly those rows
    K = case['K']
    n_const = 0
    for k, (i, j) in enumerate(zip(res['i'].tolist(), res['j'].tolist())):
        jb = j - n_a
        if numpy.isnan(res['gap'][k]):
            continue
        if case['copied'].get(jb) == i:
            assert res['gap'][k] == 0.0 and res['row'][k] == 0 and numpy.all(res['ranges'][k] == 0.0), (i, jb)
            n_const += K
        elif case['shifted'] == (jb, i):
            d = laws[i][:, 0] - laws[j][:, 0]
            assert res['gap'][k] == numpy.abs(d).max() and res['row'][k] == int(numpy.argmax(numpy.abs(d))), (i, jb)
            assert numpy.array_equal(res['ranges'][k], numpy.column_stack([d, d]))
            n_const += K
    assert any(case['copied'].get(j - n_a) == i for i, j in meeting) and (case['shifted'][1], case['shifted'][0] + n_a) in meeting
    st = res['stats']
    assert st['constant_rows'] == n_const == sum(w['constant'] for w in want.values())
    assert st['pairs'] == len(cand) and st['meets'] == len(meeting) and st['wide'] == 0
    assert st['lps'] == len(cand) + 2 * (K * len(meeting) - n_const) == sum(w['lps'] for w in want.values())


@pytest.mark.parametrize('n', [2, 16])
def test_padded_to_the_lds_limit(n):
    """every region filled to 256 rows by redundant rows: 512 rows per pair, and the answers of the unpadded set"""
    case = cases.padded(n)
    assert all(len(p) == cases.PAD_TO for p in case['polys_a'] + case['polys_b'])
    polys, laws, n_a, res = _run_set(case)
    plain = cases.table(cases.synthetic(n))[0]
    _, knife = _against_reference(plain, laws, res)       # the redundant rows change no LP: the reference runs on the cells as they were
    assert knife == 0
    assert res['stats']['meets'] == cases.SHAPES[n][3] and res['stats']['wide'] == 0
    # and the witnesses satisfy the padded rows too
    for k in numpy.flatnonzero(~numpy.isnan(res['gap'])):
        _witness_holds(polys, laws, int(res['i'][k]), int(res['j'][k]), int(res['row'][k]), res['witness'][k], res['gap'][k])


# ---- 5. self-comparison ----------------------------------------------------------------------------------------------------------------
def test_self_comparison_runs_no_law_lp():
    sol = _double_integrator(3)
    g = sol.compare(sol, coverage=True)
    assert g.max_gap == 0.0 and g.equal(0.0) and g.wide == 0
    assert len(g.unmatched_a) == 0 and len(g.unmatched_b) == 0
    assert g.stats['lps'] == g.stats['pairs'] == len(g.i)            # the radius runs alone
    n_x = numpy.asarray(sol.critical_regions[0].A).shape[0]
    assert g.stats['constant_rows'] == n_x * g.stats['meets'] and g.stats['meets'] >= len(sol)
    assert numpy.all(g.meets[g.i == g.j])
    assert numpy.all(numpy.abs(g.covered_a - 1.0) <= 1e-9) and numpy.all(numpy.abs(g.covered_b - 1.0) <= 1e-9)


# ---- 6. merged against source ----------------------------------------------------------------------------------------------------------
def _theta_bounds(prog):
    """max |theta_t| over {A_t theta <= b_t}, per coordinate"""
    A_t, b_t = numpy.asarray(prog.A_t, dtype=float), numpy.asarray(prog.b_t, dtype=float).reshape(-1)
    n = A_t.shape[1]
    out = numpy.zeros(n)
    for t in range(n):
        for sign in (1.0, -1.0):
            r = linprog(-sign * numpy.eye(n)[t], A_ub=A_t, b_ub=b_t, bounds=[(None, None)] * n, method='highs-ds')
            assert r.status == 0
            out[t] = max(out[t], -r.fun)
    return out


def test_merged_against_its_source():
    sol = _double_integrator(3)
    law_tol = 1e-8
    m = sol.merge_regions(outputs=[0], law_tol=law_tol)
    g = m.compare(sol, outputs=[0], ranges=True)
    polys, laws, n_a = _tables(m, sol, [0], [0])
    res = {'i': g.i, 'j': g.j + n_a, 'radius': g.radius, 'gap': g.gap, 'row': g.row, 'witness': g.witness, 'flag': g.flag, 'ranges': g.ranges}
    _against_reference(polys, laws, res)
    # law_groups: a member's law agrees with the group's first law within law_tol (1 + max |first law|) in every entry of [A | b], so
    # |delta(theta)| <= law_tol (1 + L) (1 + sum_t |theta_t|); the factor 2 leaves room for the region's own rounding
    L = float(numpy.max(numpy.abs(laws)))
    bound = 2.0 * law_tol * (1.0 + L) * (1.0 + float(_theta_bounds(sol.program).sum()))
    assert g.max_gap <= bound, (g.max_gap, bound)
    assert len(g.unmatched_a) == 0 and len(g.unmatched_b) == 0 and g.wide == 0


# ---- 7. two different controllers --------------------------------------------------------------------------------------------------------
def test_two_horizons_sandwich():
    a, b = _double_integrator(2), _double_integrator(3)
    g = a.compare(b, outputs=[0])
    assert g.wide == 0 and g.max_gap > 0.0
    rng = numpy.random.default_rng(5)
    pts = rng.uniform(-4.0, 4.0, size=(20_000, 2))
    xa, ra = a.evaluate_batch(pts)
    xb, rb = b.evaluate_batch(pts)
    both = (ra >= 0) & (rb >= 0)
    assert both.sum() > 100
    sampled = numpy.abs(xa[both, 0] - xb[both, 0])
    assert sampled.max() <= g.max_gap + 1e-9, (sampled.max(), g.max_gap)
    polys, laws, n_a = _tables(a, b, [0], [0])
    k = g.argmax
    _witness_holds(polys, laws, int(g.i[k]), int(g.j[k]) + n_a, int(g.row[k]), g.witness[k], g.max_gap)
    assert g.row[k] == 0


# ---- 8. determinism and order ----------------------------------------------------------------------------------------------------------
def test_reruns_and_permutations_are_bit_identical():
    polys, laws, n_a = cases.table(cases.synthetic(3))
    off, ef = cases.csr(polys)
    xs, box, status, _ = _lib.merge_regions(off, ef)
    pa, pb = cmp.cross_box_pairs(box[:n_a], status[:n_a] == 0, box[n_a:], status[n_a:] == 0, TOL)
    pb = pb + n_a
    keys = ('radius', 'gap', 'row', 'witness', 'flag', 'ranges')
    first = cmp.law_gap_pairs(off, ef, laws, pa, pb, tol=TOL, xs=xs, ranges=True)
    again = cmp.law_gap_pairs(off, ef, laws, pa, pb, tol=TOL, xs=xs, ranges=True)
    perm = numpy.random.default_rng(1).permutation(len(pa))
    mixed = cmp.law_gap_pairs(off, ef, laws, pa[perm], pb[perm], tol=TOL, xs=xs, ranges=True)
    for key in keys:
        assert first[key].tobytes() == again[key].tobytes(), key
        assert first[key][perm].tobytes() == mixed[key].tobytes(), key
    counters = lambda res: {k: v for k, v in res['stats'].items() if not k.endswith('_ms')}
    assert counters(first) == counters(again) == counters(mixed)


# ---- 9. refusals of the library ------------------------------------------------------------------------------------------------------------
def test_library_refuses_bad_arguments():
    polys, laws, _ = cases.open_half_strip()
    off, ef = cases.csr(polys)
    xs = numpy.full((3, 2), 0.5)
    ok = lambda **kw: _lib.law_gap_pairs(kw.get('off', off), kw.get('ef', ef), kw.get('laws', laws), kw.get('xs', xs), kw.get('pa', [0, 2]),
                                         kw.get('pb', [1, 2]), kw.get('tol', TOL))
    radius, gap, row, witness, rng, flag, st = ok()
    assert rng is None and gap[0] == numpy.inf and gap[1] == 0.0 and st['pairs'] == 2       # (2, 2): a region against itself
    nan_laws, nan_xs, bad_rows, inf_rows = laws.copy(), xs.copy(), ef.copy(), ef.copy()
    nan_laws[1, 0, 2], nan_xs[2, 1], inf_rows[0, 0] = numpy.nan, numpy.inf, numpy.inf
    bad_rows[1, 1:] *= 2.0
    wide_ef = numpy.column_stack([numpy.ones(17), numpy.eye(17)])
    for kw, text in (({'laws': nan_laws}, 'laws must be finite'), ({'xs': nan_xs}, 'xs must be finite'), ({'ef': bad_rows}, 'unit normals'),
                     ({'ef': inf_rows}, 'unit normals'), ({'tol': -1e-9}, 'tol must be finite'), ({'tol': numpy.nan}, 'tol must be finite'),
                     ({'pa': [0, 3]}, 'out of range'), ({'pb': [-1, 1]}, 'out of range'),
                     ({'laws': numpy.zeros((3, 257, 3))}, r'n_out must lie in 1\.\.256'),
                     ({'off': numpy.array([0, 257, 514, 771]), 'ef': numpy.tile(ef[:1], (771, 1))}, r'1\.\.256 rows'),
                     ({'off': numpy.array([0, 0, 1, 9]), 'ef': numpy.tile(ef[:1], (9, 1))}, r'1\.\.256 rows'),
                     ({'off': numpy.arange(18), 'ef': wide_ef, 'laws': numpy.zeros((17, 1, 18)), 'xs': numpy.zeros((17, 17))}, r'n_t must lie in 1\.\.16')):
        with pytest.raises(_lib.MpcError, match=text):
            ok(**kw)
    # a missing array, straight at the C entry point
    L = _lib.load()
    import ctypes
    p32, pd = numpy.zeros(1, dtype=numpy.int32), numpy.zeros(4)
    args = [0, 2, 1, 3, _lib._ptr(off), _lib._ptr(ef), _lib._ptr(numpy.ascontiguousarray(laws)), _lib._ptr(xs), 1, _lib._ptr(p32), _lib._ptr(p32),
            TOL, _lib._ptr(pd), _lib._ptr(pd), _lib._ptr(p32), _lib._ptr(pd), None, _lib._ptr(p32), None, None]
    assert L.mpc_law_gap_pairs(*args) == _lib.MPC_OK
    for hole in (6, 7, 9, 10, 12, 13, 14, 15, 17):
        broken = list(args)
        broken[hole] = None
        assert L.mpc_law_gap_pairs(*broken) == _lib.MPC_ERR_INVALID, hole
        assert b'missing array' in L.mpc_last_error(None)
    none = list(args)
    none[8] = 0
    none[9] = none[10] = None
    assert L.mpc_law_gap_pairs(*none) == _lib.MPC_OK                  # n_pairs == 0: no launch, nothing else is looked at
