"""The list scan, the evaluation, the adjacency walk with its fallbacks, and the facet centres against references that are not device
kernels (tests/locate_reference.py): synthetic inputs at the C-ABI level, no program is solved.

Lattice cases are compared with equality (regions and x), and no point is left out; wide cases use the derived bounds of
locate_wide; facet centres the LP tolerance 1e-9 of the parameter-point LP tests.  Every walk case is a lattice case: the walk has
to return the scan's answer."""
import functools
import itertools

import numpy
import pytest

import locate_reference as ref
from locate_reference import LATTICE, TOL
from ppopt_amd import _lib

pytestmark = pytest.mark.gpu

MODES = [dict(), dict(inclusive=True), dict(overlapping=True), dict(overlapping=True, inclusive=True)]


def _locator(row_off, ef, xlaw, Q=None, c=None, H=None):
    return _lib.Locator(row_off, ef, xlaw, Q, c, H)


def _check_exact(row_off, ef, xlaw, theta, Q=None, c=None, H=None, tols=(0.0, TOL), modes=MODES, loc=None, **flags):
    """device == reference, regions and x, for every tolerance and rule; the data are certified exact first.  Returns the answers."""
    row, xb, ob = ref.exact_bits(ef, xlaw, theta, max(tols), Q, c, H)
    assert row <= 53 and xb <= 53 and (ob <= 53 or not any(m.get('overlapping') for m in modes)), (row, xb, ob)
    own = loc is None
    loc = loc or _locator(row_off, ef, xlaw, Q, c, H)
    out = []
    try:
        for tol in tols:
            for mode in modes:
                got_r, got_x = loc.query(theta, tol, **mode, **flags)
                want_r, want_x = ref.locate(row_off, ef, xlaw, theta, tol, Q=Q, c=c, H=H, **mode)
                bad = numpy.flatnonzero(got_r != want_r)
                assert bad.size == 0, (tol, mode, flags, bad.size, bad[:8], got_r[bad[:8]], want_r[bad[:8]], theta[bad[:8]])
                assert numpy.array_equal(got_x, want_x, equal_nan=True), (tol, mode)
                out.append(want_r)
    finally:
        if own:
            loc.close()
    return out


def _slabs(n_t, counts, lo=-4.0, width=0.5):
    """disjoint slabs along axis 0, slab r with counts[r] rows (its box rows repeated): regions and one interior point each"""
    regs, mids = [], []
    for r, k in enumerate(counts):
        a, b = numpy.full(n_t, -4.0), numpy.full(n_t, 4.0)
        a[0], b[0] = lo + r * width, lo + (r + 1) * width
        regs.append(ref.padded(ref.box_rows(a, b), k))
        mids.append(0.5 * (a + b))
    return regs, numpy.array(mids)


def _laws(seed, R, n_x, n_t):
    return ref.lattice_laws(numpy.random.default_rng(seed), R, n_x, n_t, 0.25, 2.0)


# ---- the scan and the evaluation: shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_x', [1, 3, 17])
@pytest.mark.parametrize('n_t', [1, 4, 5, 8, 9, 16])
def test_widths(n_t, n_x):
    """both edges of the NT = 4 / 8 / 16 instantiations: fine lattice without an objective, coarse lattice with Q, c and H"""
    row_off, ef, xlaw, Q, c, H, theta = ref.lattice_case(1000 + 20 * n_t + n_x, n_t, n_x, False)
    seen = _check_exact(row_off, ef, xlaw, theta)
    assert len(numpy.unique(seen[0])) >= 4
    row_off, ef, xlaw, Q, c, H, theta = ref.lattice_case(2000 + 20 * n_t + n_x, n_t, n_x, True)
    _check_exact(row_off, ef, xlaw, theta, Q, c, H)


@pytest.mark.parametrize('m', [0, 1, 63, 64, 65, 255, 256, 257, 513])
def test_point_counts(m):
    """inside one block wave 0 finishes at region 0, wave 1 is spread over all regions, wave 2 has no region and wave 3 needs the last
    one: the early exit of one wave must not disturb the barriers and tiles of the others"""
    regs, mids = _slabs(4, [8] * 40)     # 320 rows: two tiles
    row_off, ef = ref.stack(regs, 4)
    p = numpy.arange(m)
    wave = (p % 256) // 64
    target = numpy.select([wave == 0, wave == 1, wave == 3], [0, p % 40, 39], default=-1)
    theta = numpy.where(target[:, None] >= 0, mids[numpy.maximum(target, 0)], 5.0) + LATTICE * (p % 7)[:, None]
    seen = _check_exact(row_off, ef, _laws(m, 40, 3, 4), theta.reshape(m, 4))
    assert numpy.array_equal(seen[0], target)


@pytest.mark.parametrize('total', [255, 256, 257, 512, 513])
def test_total_rows_at_the_tile_edges(total):
    counts = [7, total - 41, 30, 4]
    regs, mids = _slabs(2, counts)
    row_off, ef = ref.stack(regs, 2)
    assert row_off[-1] == total
    rng = numpy.random.default_rng(total)
    theta = numpy.vstack([mids[rng.integers(0, 4, size=200)] + ref.lattice(rng, (200, 2), -0.25, 0.25),     # slab edges included
                          ref.lattice(rng, (59, 2), -5, 5, 0.25)])
    seen = _check_exact(row_off, ef, _laws(total, 4, 3, 2), theta)
    assert set(seen[0]) == {-1, 0, 1, 2, 3}


@pytest.mark.parametrize('first', [250, 244])
def test_a_region_across_and_up_to_a_tile_edge(first):
    """region 1 has 12 rows: six of theta_0 <= 1, then six of theta_1 <= 1.  After 250 rows of region 0 it straddles the edge of the
    first tile (a point may pass every row of one tile and fail only in the other); after 244 it ends exactly on row 255."""
    regs, mids = _slabs(2, [first])
    r1 = numpy.array([[1.0, 1.0, 0.0]] * 6 + [[1.0, 0.0, 1.0]] * 6)
    row_off, ef = ref.stack([regs[0], r1, ref.box_rows([-4.0, -4.0], [4.0, 4.0])], 2)
    base = numpy.array([[0.0, 0.0], [0.0, 2.0], [2.0, 0.0], [2.0, 2.0], [-3.75, 0.0], [0.0, 5.0], [1.0, 1.0], [1.0 + TOL, 0.0], [0.0, 1.0 + TOL]])
    theta = numpy.vstack([base + LATTICE * k for k in range(-7, 8)])     # 135 points: three waves
    seen = _check_exact(row_off, ef, _laws(first, 3, 1, 2), theta)
    assert seen[0][:6].tolist() == [1, 2, 2, 2, 0, -1]     # the base points moved by -7 lattice steps, strict, tol 0


def test_a_jump_over_two_tiles_to_the_last_region():
    """a 600-row region that every lane leaves at its first row: the next row of the wave lies two tiles ahead, in the last region"""
    regs, mids = _slabs(2, [4])
    big = numpy.vstack([[[-100.0, 1.0, 0.0]], ref.padded(ref.box_rows([-4.0, -4.0], [4.0, 4.0]), 599)])
    last = ref.box_rows([0.0, 0.0], [2.0, 2.0])
    row_off, ef = ref.stack([regs[0], big, last], 2)
    assert row_off.tolist() == [0, 4, 604, 608]
    rng = numpy.random.default_rng(5)
    theta = numpy.vstack([ref.lattice(rng, (100, 2), -0.5, 2.5, 0.25), mids[[0] * 20], ref.lattice(rng, (80, 2), -4, 4)])
    seen = _check_exact(row_off, ef, _laws(6, 3, 3, 2), theta)
    assert set(seen[0]) == {-1, 0, 2}
    # without region 0 no lane is ever inside a region before the jump
    row_off, ef = ref.stack([big, last], 2)
    assert set(_check_exact(row_off, ef, _laws(7, 2, 3, 2), theta)[0]) == {-1, 1}


def test_regions_without_rows():
    none = numpy.zeros((0, 3))
    box = lambda lo, hi: ref.box_rows([lo, lo], [hi, hi])
    regs = [none, box(-1.0, 0.0), none, none, box(0.0, 1.0), box(-2.0, 2.0), none]
    row_off, ef = ref.stack(regs, 2)
    rng = numpy.random.default_rng(8)
    theta = ref.lattice(rng, (300, 2), -2.5, 2.5, 0.125)
    seen = _check_exact(row_off, ef, _laws(8, 7, 3, 2), theta)
    assert set(seen[0]) == {-1, 1, 4, 5} and set(seen[2]) == {-1, 5}
    # no region has a row; there is no region; there is no point
    for R in (3, 0):
        row_off, ef = ref.stack([none] * R, 2)
        laws = _laws(9, R, 3, 2).reshape(R, 3, 3)
        assert set(_check_exact(row_off, ef, laws, theta)[0]) == {-1}
    loc = _locator(*ref.stack(regs, 2), _laws(8, 7, 3, 2))
    for mode in MODES:
        r, x = loc.query(numpy.zeros((0, 2)), TOL, **mode)
        assert r.shape == (0,) and x.shape == (0, 3)
    loc.close()


# ---- the rules, on the lattice -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tol', [0.0, TOL])
def test_points_on_and_next_to_facets(tol):
    """E theta - f exactly -2^-12, 0, tol - 2^-12, tol, tol + 2^-12 on one row and on two rows at once: strict excludes tol, inclusive
    includes it"""
    ds = sorted({-LATTICE, 0.0, tol - LATTICE, tol, tol + LATTICE})
    inner = numpy.vstack([ref.box_rows([-1.0] * 3, [1.0] * 3), [[1.5, 1.0, 1.0, 0.0]]])
    row_off, ef = ref.stack([inner, ref.box_rows([-2.0] * 3, [2.0] * 3)], 3)
    pts = []
    for edge in (1.0, 2.0):
        for d in ds:
            pts += [[edge + d, 0, 0], [0, 0, -edge - d], [0, edge + d, 0]]
        for d1, d2 in itertools.product(ds, ds):
            pts += [[edge + d1, 0, edge + d2], [-edge - d1, edge + d2, 0]]
    for d in ds:
        pts.append([0.75 + d, 0.75, 0])                       # the oblique row alone
    for d1, d2 in itertools.product(ds, ds):
        pts.append([1.0 + d1, 0.5 + d2 - d1, 0])              # the oblique row and theta_0 <= 1
    theta = numpy.array(pts, dtype=float)
    strict, incl = _check_exact(row_off, ef, _laws(3, 2, 3, 3), theta, tols=(tol,), modes=MODES[:2])
    on = numpy.array([1.0 + tol, 0.0, 0.0])
    k = int(numpy.flatnonzero(numpy.all(theta == on, axis=1))[0])
    assert strict[k] == 1 and incl[k] == 0
    _check_exact(row_off, ef, _laws(3, 2, 3, 3), theta, tols=(tol,), modes=MODES[2:])


@pytest.mark.parametrize('order', ['inner_first', 'outer_first'])
def test_first_match_among_duplicate_and_nested_regions(order):
    box = lambda h: ref.box_rows([-h, -h], [h, h])
    regs = [box(0.5), box(1.0), box(1.0), box(2.0), ref.box_rows([0.0, 0.0], [3.0, 3.0])]
    if order == 'outer_first':
        regs = regs[::-1]
    row_off, ef = ref.stack(regs, 2)
    theta = ref.lattice(numpy.random.default_rng(4), (400, 2), -2.5, 3.5, 0.125)
    seen = _check_exact(row_off, ef, _laws(4, 5, 3, 2), theta)
    first, last = set(seen[0]), set(seen[2])     # without an objective every tie goes to the last containing region
    assert (first, last) == (({-1, 0, 1, 3, 4}, {-1, 3, 4}) if order == 'inner_first' else ({-1, 0, 1}, {-1, 0, 1, 3, 4}))


@pytest.mark.parametrize('terms', ['none', 'c', 'H', 'Q', 'QcH'])
def test_overlap_picks_the_lowest_objective(terms):
    """exact ties (equal laws: the later region wins) and strictly lower objectives earlier and later in the list"""
    rng = numpy.random.default_rng(sum(map(ord, terms)))
    n_t, n_x, R = 2, 3, 8
    regs = [ref.box_rows(lo, lo + 3.0) for lo in ref.lattice(rng, (R, n_t), -3, 0, 0.25)]
    row_off, ef = ref.stack(regs, n_t)
    xlaw = ref.lattice_laws(rng, R, n_x, n_t, 0.25, 2.0)
    xlaw[5], xlaw[6] = xlaw[1], xlaw[2]
    Q = ref.lattice(rng, (n_x, n_x), -2, 2, 0.25) if 'Q' in terms else None
    c = ref.lattice(rng, n_x, -2, 2, 0.25) if 'c' in terms else None
    H = ref.lattice(rng, (n_x, n_t), -2, 2, 0.25) if 'H' in terms else None
    theta = ref.lattice(rng, (500, n_t), -3.5, 3.5, 0.0625)
    first, _, low, _ = _check_exact(row_off, ef, xlaw, theta, Q, c, H, tols=(TOL,))
    inside = numpy.array([ref.locate(row_off[r:r + 2] - row_off[r], ef[row_off[r]:row_off[r + 1]], xlaw[r:r + 1], theta, TOL)[0] == 0
                          for r in range(R)])
    last = numpy.where(inside.any(axis=0), R - 1 - numpy.argmax(inside[::-1], axis=0), -1)
    many = inside.sum(axis=0) >= 2
    if terms == 'none':
        assert numpy.array_equal(low, last)
    else:
        assert (low[many] == first[many]).any() and (low[many] == last[many]).any() and ((low != first) & (low != last)).any()
    tie = many & ((low == 5) | (low == 6))
    assert tie.any() and not ((low == 1) & inside[5]).any() and not ((low == 2) & inside[6]).any()


def test_nan_parameters():
    """a NaN component: no region and NaN x under every rule, and the other lanes of the wave are not affected"""
    row_off, ef, xlaw, Q, c, H, theta = ref.lattice_case(77, 5, 3, True)
    theta = numpy.vstack([theta, theta])[:130].copy()
    clean = theta.copy()
    for p, t in ((0, 0), (5, 4), (63, 2), (64, 1), (129, 3)):
        theta[p, t] = numpy.nan
    theta[70] = numpy.nan
    nan_rows = numpy.isnan(theta).any(axis=1)
    loc = _locator(row_off, ef, xlaw, Q, c, H)
    seen = _check_exact(row_off, ef, xlaw, theta, Q, c, H, loc=loc)
    for want, (tol, mode) in zip(seen, itertools.product((0.0, TOL), MODES)):
        assert numpy.all(want[nan_rows] == -1)
        assert numpy.array_equal(want[~nan_rows], loc.query(clean, tol, **mode)[0][~nan_rows])
    loc.close()


# ---- random float64 data against long double ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wide(shape):
    return ref.wide_case(shape)


@pytest.mark.parametrize('mode', ['strict', 'inclusive', 'overlap'])
@pytest.mark.parametrize('shape', sorted(ref.WIDE_CASES))
def test_wide_data(shape, mode):
    case = _wide(shape)
    flags = {'strict': {}, 'inclusive': {'inclusive': True}, 'overlap': {'overlapping': True}}[mode]
    args = (case['row_off'], case['ef'], case['xlaw'])
    want_r, want_x, keep, x_bound = ref.locate_wide(*args, case['theta'], case['tol'], Q=case['Q'], c=case['c'], H=case['H'], **flags)
    assert numpy.mean(~keep) <= 0.01
    loc = _locator(*args, case['Q'], case['c'], case['H'])
    got_r, got_x = loc.query(case['theta'], case['tol'], **flags)
    loc.close()
    assert numpy.array_equal(got_r[keep], want_r[keep]), int(numpy.sum(got_r[keep] != want_r[keep]))
    hit = keep & (want_r >= 0)
    assert hit.sum() >= 400
    assert numpy.all(numpy.abs(got_x[hit] - want_x[hit].astype(float)) <= x_bound[hit])
    none = keep & (want_r < 0)
    assert none.any() and numpy.all(numpy.isnan(got_x[none]))


# ---- the walk ----------------------------------------------------------------------------------------------------------------------
def _walk_locator(b, g, n_x=2, seed=0):
    xlaw = _laws(seed, len(b['cells']), n_x, g.n_t)
    loc = _locator(b['row_off'], b['ef'], xlaw)
    assert loc.set_adjacency(b['masks'], b['row_info'], g.n_c)
    return loc, xlaw


def _check_walk(b, g, theta, tols=(TOL, 0.0), unresolved=None):
    """unresolved: receives the number of points that the last query handed to the exhaustive pass"""
    loc, xlaw = _walk_locator(b, g)
    try:
        want = _check_exact(b['row_off'], b['ef'], xlaw, theta, tols=tols, modes=MODES[:1], loc=loc, walk=True)
        if unresolved is not None:
            unresolved.append(loc.last_unresolved)
        return want
    finally:
        loc.close()


def _outside_points(g, rng):
    """beyond the outer box on every axis by 0.5, 2, 5 (less than 10) and 20, 1024 (more than 10) tol"""
    pts = []
    for a in range(g.n_t):
        for sign in (-1.0, 1.0):
            for k in (0.5, 2.0, 5.0, 20.0, 1024.0):
                p = g.centre(g.all_cells()[int(rng.integers(len(g.all_cells())))], rng)
                p[a] = sign * ((g.cuts[a][-1] if sign > 0 else -g.cuts[a][0]) if a in g.axes else g.outer) + sign * k * TOL
                pts.append(p)
    return numpy.array(pts)


NEAR = [0.0] + ref.walk_offsets()      # 0 and +-{1/2, 1, 2} tol


@pytest.mark.parametrize('seed', [1, 2])
@pytest.mark.parametrize('name', sorted(ref.GRIDS))
def test_walk_is_the_scan_on_grids(name, seed):
    """cell interiors, points at +-{1/2, 1, 2} tol from every facet, within tol of every corner shared by four (eight) cells, outside
    the parameter set, and a NaN; mask words 2 (ids across bit 63 / 64) and 4 (ids in words 2 and 3)"""
    g = ref.GRIDS[name]()
    b = g.build(g.shuffled(seed))
    rng = numpy.random.default_rng(seed)
    theta = numpy.vstack([numpy.array([g.centre(cell, rng) for cell in g.all_cells()]), g.facet_points(ref.walk_offsets(), rng),
                          g.corner_points(NEAR, rng), _outside_points(g, rng), numpy.full((1, g.n_t), numpy.nan)])
    want = _check_walk(b, g, theta)[0]
    assert set(want[want >= 0]) == set(range(len(b['cells'])))


def test_walk_at_the_corner_of_the_worked_example():
    """3 x 2 boxes; the point (-tol/2, -tol/2) lies strictly in A (region 2) and within tol in D (region 1), which is not a neighbour
    of A across a row: the scan answers 1"""
    g = ref.Grid(2, {0: [-4.0, -2.0, 0.0, 4.0], 1: [-4.0, 0.0, 4.0]}, {0: 0, 1: 70}, 128, 2)
    b = g.build([(0, 0), (2, 1), (1, 0), (2, 0), (1, 1), (0, 1)])
    theta = numpy.vstack([[[-TOL / 2, -TOL / 2]], g.corner_points(NEAR)])
    want = _check_walk(b, g, theta)
    assert want[0][0] == 1 and want[1][0] == 2


@pytest.mark.parametrize('name', ['2d', '3d'])
def test_walk_with_every_corner_cell_first(name):
    """around one corner, each of the four (eight) cells in turn is the earliest of the list, right behind a far starting region"""
    g = ref.GRIDS[name]()
    corner = tuple(k // 2 for k in g.shape)
    around = [tuple(c - d for c, d in zip(corner, dd)) for dd in itertools.product((0, 1), repeat=len(g.shape))]
    rest = [cell for cell in g.shuffled(9) if cell not in around]
    theta = g.corner_points(NEAR)
    for lead in around:
        cells = [rest[0], lead] + rest[1:] + [cell for cell in around[::-1] if cell != lead]
        want = _check_walk(g.build(cells), g, theta, tols=(TOL,))[0]
        assert (want == 1).sum() >= 3 ** len(g.shape)


def test_walk_with_unknown_rows_and_holes():
    """cells whose rows are of kind 3 and cells missing from the list: the walk hands the points to the exhaustive pass where it cannot
    certify the first match; points in and beyond the holes"""
    g = ref.GRIDS['2d']()
    cells = g.shuffled(5)
    holes = set(cells[3::11]) | {(0, 0), (11, 5), (5, 5), (5, 6)}
    kept = [cell for cell in cells if cell not in holes]
    unknown = set(kept[2::7])
    b = g.build(kept, unknown=unknown)
    rng = numpy.random.default_rng(5)
    theta = numpy.vstack([numpy.array([g.centre(cell) for cell in g.all_cells()]), g.facet_points(ref.walk_offsets()), g.corner_points(NEAR),
                          _outside_points(g, rng)])
    want = _check_walk(b, g, theta)[0]
    centres = want[:len(g.all_cells())]
    assert (centres < 0).sum() == len(holes) and set(centres[centres >= 0]) == set(range(len(kept)))


@pytest.mark.parametrize('m', [20000, 5000])
def test_walk_fallbacks_by_size(m):
    """region 0 has only rows of kind 3, so every point is left unresolved: 20,000 of them go to the list scan, 5,000 (at most 16,384) to
    the pass over every (point, region) pair"""
    g = ref.GRIDS['3d']()
    cells = g.shuffled(6)
    b = g.build(cells, unknown={cells[0]})
    rng = numpy.random.default_rng(m)
    theta = numpy.vstack([ref.lattice(rng, (m - 2000, g.n_t), -3.5, 3.5), g.corner_points(NEAR, rng)[:2000]])
    unresolved = []
    want = _check_walk(b, g, theta, tols=(TOL,), unresolved=unresolved)[0]
    assert len(want) == m and (want == 0).any() and (want < 0).any() and len(set(want)) == len(cells) + 1
    # the walk starts in region 0 and can leave it through no row: every point that it does not certify there is unresolved, at
    # least those of the other regions and those outside, and the count decides between the two passes (16,384)
    assert (want != 0).sum() <= unresolved[0] <= m
    assert unresolved[0] > 16384 if m == 20000 else 0 < unresolved[0] <= 16384


def test_walk_flag_is_ignored_with_the_other_rules():
    g = ref.GRIDS['2d']()
    b = g.build(g.shuffled(4))
    loc, xlaw = _walk_locator(b, g)
    theta = numpy.vstack([g.corner_points(NEAR), g.facet_points(ref.walk_offsets())])
    _check_exact(b['row_off'], b['ef'], xlaw, theta, modes=MODES[1:], loc=loc, walk=True)
    loc.close()


# ---- facet centres -----------------------------------------------------------------------------------------------------------------
def _check_facets(row_off, ef, want_status, want_radius):
    """status equal; radius within the LP tolerance; the centre a certificate of that radius; zeros where not optimal"""
    centre, radius, status = _lib.facet_centres(ef, row_off)
    assert numpy.array_equal(status, want_status), numpy.flatnonzero(status != want_status)[:10]
    for r in range(len(row_off) - 1):
        rows = ef[row_off[r]:row_off[r + 1]]
        fmax = numpy.max(numpy.abs(rows[:, 0]))
        for q in range(len(rows)):
            k = row_off[r] + q
            if want_status[k] != ref.LP_OPTIMAL:
                assert radius[k] == 0.0 and numpy.all(centre[k] == 0.0)
                continue
            assert abs(radius[k] - want_radius[k]) <= ref.LP_TOL * max(1.0, abs(want_radius[k]), fmax), (r, q, radius[k], want_radius[k])
            assert ref.certificate_violation(rows, q, centre[k], radius[k]) <= ref.LP_TOL, (r, q)
    return centre, radius, status


@pytest.mark.parametrize('n', range(1, 17))
def test_facets_of_boxes_and_simplices(n):
    """closed forms: a box facet has half the shortest other side (at most the box's extent across it), a simplex facet
    1 / (n - 1 + sqrt n) or 1 / n"""
    rng = numpy.random.default_rng(n)
    sides = rng.integers(1, 9, size=n) * 0.25
    lo = rng.integers(-8, 8, size=n) * 0.5
    row_off, ef = ref.stack([ref.box_rows(lo, lo + sides), ref.simplex_rows(n), ref.box_rows(-numpy.ones(n), numpy.ones(n))], n)
    want = numpy.r_[[ref.box_facet_radius(sides, k // 2) for k in range(2 * n)], ref.simplex_radii(n),
                    [ref.box_facet_radius([2.0] * n, 0)] * (2 * n)]
    _check_facets(row_off, ef, numpy.zeros(len(ef), dtype=numpy.int32), want)


@functools.lru_cache(maxsize=None)
def _tangent(n, m, seed):
    rows = ref.tangent_polytope(numpy.random.default_rng(seed), n, m)
    return rows, ref.facet_centres(*ref.stack([rows], n))


@pytest.mark.parametrize('n,m,seed', ref.FACET_SHAPES)
def test_facets_by_row_count(n, m, seed):
    """63, 64, 127 and 128 rows: with the row of the radius the tableau has 64, 65, 128 and 129, across the 64-lane strides"""
    rows, (st, ce, ra) = _tangent(n, m, seed)
    _check_facets(*ref.stack([rows], n), st, ra)


WEDGE = numpy.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 1.0, 0.0]])                                   # two rows, both facets unbounded
REDUNDANT = numpy.vstack([ref.box_rows([-1.0] * 3, [1.0] * 3), [[5.0, 1.0, 0.0, 0.0]]])              # the last row is strictly redundant
HALF_STRIP = numpy.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 1.0, 0.0], [1.0, 0.0, -1.0, 0.0], [3.0, 0.0, 0.0, 1.0], [3.0, 0.0, 0.0, -1.0]])


def test_facets_of_a_mixed_batch():
    """2 to 128 rows in one launch (the LDS layout follows the largest), optimal, infeasible and unbounded facets side by side"""
    polys = [_tangent(3, 63, 2)[0], ref.box_rows([-1.0] * 3, [1.0] * 3), _tangent(3, 128, 5)[0], WEDGE, REDUNDANT, _tangent(3, 64, 3)[0],
             ref.simplex_rows(3), HALF_STRIP]
    row_off, ef = ref.stack(polys, 3)
    st, ce, ra = ref.facet_centres(row_off, ef)
    assert {ref.LP_OPTIMAL, ref.LP_INFEASIBLE, ref.LP_UNBOUNDED} == set(st)
    _check_facets(row_off, ef, st, ra)


def test_facet_status_cases():
    for poly, want in ((WEDGE, [ref.LP_UNBOUNDED] * 2), (REDUNDANT, [ref.LP_OPTIMAL] * 6 + [ref.LP_INFEASIBLE]),
                       (HALF_STRIP, [ref.LP_OPTIMAL] * 5), (ref.box_rows([-1.0], [1.0]), [ref.LP_OPTIMAL] * 2)):
        n = poly.shape[1] - 1
        row_off, ef = ref.stack([poly], n)
        st, ce, ra = ref.facet_centres(row_off, ef)
        assert st.tolist() == want
        _check_facets(row_off, ef, st, ra)


def test_facets_of_9600_rows():
    """more facets than the launch has wavefronts, so every wavefront takes further work: 12 base polytopes of 8 rows, each moved and
    scaled by powers of two 100 times; the expected radius is the base's, scaled"""
    orthant = numpy.array([[0.0, -1, 0, 0], [0.0, 0, -1, 0], [0.0, 0, 0, -1], [1.0, -1, -1, 0], [1.0, 0, -1, -1], [1.0, -1, 0, -1],
                           [1.0, -1, -1, -1], [2.0, -1, 0, 0]])
    bases = [ref.tangent_polytope(numpy.random.default_rng(40 + k), 3, 8) for k in range(10)]
    bases += [numpy.vstack([ref.box_rows([-1.0] * 3, [1.0] * 3), [[4.0, 1.0, 1.0, 0.0], [3.0, 0.0, 0.0, -1.0]]]), orthant]
    solved = [ref.facet_centres(*ref.stack([rows], 3)) for rows in bases]
    assert all(numpy.all((st != ref.LP_OPTIMAL) | (ra > 1e-6)) for st, ce, ra in solved)
    rng = numpy.random.default_rng(9600)
    polys, want_st, want_ra = [], [], []
    for k in range(100):
        for rows, (st, ce, ra) in zip(bases, solved):
            s, t = 2.0 ** rng.integers(-3, 4), rng.integers(-8, 9, size=3) * 2.0 ** rng.integers(-2, 2)
            polys.append(numpy.c_[s * rows[:, 0] + rows[:, 1:] @ t, rows[:, 1:]])     # {s theta + t}
            want_st.append(st)
            want_ra.append(s * ra)
    row_off, ef = ref.stack(polys, 3)
    assert len(ef) == 9600
    want_st, want_ra = numpy.concatenate(want_st), numpy.concatenate(want_ra)
    assert (want_st == ref.LP_INFEASIBLE).any() and (want_st == ref.LP_UNBOUNDED).any()
    _check_facets(row_off, ef, want_st, want_ra)
