"""Merging regions with equal laws on the device: Solution.merge_regions against the independent CPU reference on the
hand-built cases and on random partitions of polytopes up to n_theta = 16 and 256 rows, then the properties of merged solved
programs: a partition of the source with its law, the same answer as the source at 10^5 points, members inside their region and the
region inside its members, areas, pairwise maximality, no redundant rows, determinism and the search tree."""
import itertools
import warnings

import numpy
import pytest
from scipy.optimize import linprog

import merge_exact_reference as exact
import region_merge_reference as ref
from ppopt_amd import _lib
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.geometry import Polytope, hit_and_run_batch
from ppopt_amd.region_merge import MergedRegion
from ppopt_amd.solution import Solution
from test_region_merge_cpu import CASES, _Prog, _canonical

pytestmark = pytest.mark.gpu

TOL = 1e-8


def _same_as_reference(dev, want, info):
    """member lists equal and rows equal to 1e-12 after a canonical sort; exempt (and counted) when the reference met an LP value within
    its KNIFE of a threshold"""
    if info['knife']:
        return info['knife']
    assert [r.members for r in dev.critical_regions] == [r.members for r in want.critical_regions]
    for a, b in zip(dev.critical_regions, want.critical_regions):
        assert a.E.shape == b.E.shape
        numpy.testing.assert_allclose(_canonical(a.E, a.f), _canonical(b.E, b.f), rtol=0, atol=1e-12)
        numpy.testing.assert_array_equal(a.A, b.A)
        numpy.testing.assert_array_equal(a.b, b.b)
    return 0


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_the_reference_on_the_hand_built_cases(name):
    build, outputs, want_members = CASES[name]
    src = build()
    dev = src.merge_regions(outputs=outputs)
    assert [r.members for r in dev.critical_regions] == want_members
    want, info = ref.merge_reference(src, outputs)
    assert _same_as_reference(dev, want, info) == 0
    st = dev.merge_info['stats']
    assert st['regions_before'] == len(src) and st['regions_after'] == len(dev)
    assert st['rounds'] >= (1 if len(dev) < len(src) else 0)


def _irredundant(E, f):
    """rows of {E x <= f} that are facets (LP per row), or None when the cell is thin (Chebyshev radius < 1e-3)"""
    n = E.shape[1]
    nrm = numpy.linalg.norm(E, axis=1)
    r = linprog(numpy.append(numpy.zeros(n), -1.0), A_ub=numpy.column_stack([E, nrm]), b_ub=f, bounds=[(None, None)] * n + [(0, None)],
                method='highs')
    if r.status != 0 or -r.fun < 1e-3:
        return None
    keep = []
    for i in range(len(E)):
        others = [j for j in range(len(E)) if j != i]
        b = f[others]
        lp = linprog(-E[i], A_ub=numpy.vstack([E[others], E[i]]), b_ub=numpy.append(b, f[i] + 1.0), bounds=[(None, None)] * n, method='highs')
        if lp.status != 0 or -lp.fun > f[i] + 1e-9:
            keep.append(i)
    return keep


def _random_partition(rng, n, m, cuts):
    """a random polytope of m rows (unit normals, offsets around 1) cut by random hyperplanes near its centre: the cells of the
    arrangement, with their redundant rows removed, one law"""
    E0 = rng.normal(size=(m, n))
    E0 /= numpy.linalg.norm(E0, axis=1, keepdims=True)
    f0 = rng.uniform(0.8, 1.2, size=m)
    H = rng.normal(size=(cuts, n))
    H /= numpy.linalg.norm(H, axis=1, keepdims=True)
    h = rng.uniform(-0.2, 0.2, size=cuts)
    A = rng.normal(size=(2, n))
    b = rng.normal(size=(2, 1))
    regs = []
    for signs in itertools.product((1.0, -1.0), repeat=cuts):
        s = numpy.asarray(signs)
        E = numpy.vstack([E0, s[:, None] * H])
        f = numpy.concatenate([f0, s * h])
        keep = _irredundant(E, f)
        if keep is None:
            continue
        regs.append(CriticalRegion(A.copy(), b.copy(), numpy.zeros((0, n)), numpy.zeros((0, 1)), E[keep], f[keep].reshape(-1, 1), []))
    return Solution(_Prog(n), regs, point_location_tolerance=1e-5)


@pytest.mark.parametrize('n,m,cuts', [(2, 12, 3), (3, 20, 3), (6, 40, 2), (16, 60, 2), (16, 250, 1)])
def test_random_partitions_against_the_reference(n, m, cuts):
    rng = numpy.random.default_rng(1000 * n + m)
    src = _random_partition(rng, n, m, cuts)
    assert len(src) >= 2
    assert max(r.E.shape[0] for r in src.critical_regions) <= 256
    dev = src.merge_regions()
    want, info = ref.merge_reference(src)
    exempt = _same_as_reference(dev, want, info)
    assert exempt <= 2, exempt
    assert len(dev) < len(src)


# ---- solved programs -----------------------------------------------------------------------------------------------------------------
_SOLVED = {}


def _solve(name):
    if name in _SOLVED:
        return _SOLVED[name]
    import bench
    from ppopt_amd import problem_generator as pg
    from ppopt_amd.mp_solvers import mpqp_hip_combi_graph, mpqp_hip_combinatorial
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if name == 'c2x20':
            sol = solve_mpqp(bench.build_program('c2x20'), mpqp_algorithm.combinatorial)
        elif name == 'c3_l4':
            sol = mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4)
        elif name == 'c3_graph':
            # the device drivers directly: solve_mpqp flags a solution overlapping when Q is not positive definite after presolve (the
            # reference's rule), and merge_regions refuses those (test_overlapping_solved_program_is_refused)
            sol = mpqp_hip_combi_graph.solve_graph(bench.build_program('c3'))
        elif name == 'random':
            sol = mpqp_hip_combinatorial.solve(pg.generate_mpqp(4, 2, 10, seed=11))
        else:
            raise KeyError(name)
    _SOLVED[name] = sol
    return sol


# c2x20 is not here: its Q is only semidefinite, so solve_mpqp flags the solution overlapping (the reference's rule) and merge_regions
# refuses it (test_overlapping_solved_program_is_refused); the 2-D checks run on a slice of c3 instead
OUTPUTS = {'c3_l4': [0, 1], 'c3_graph': [0, 1], 'random': None}
_MERGED = {}


def _merged(name):
    if name not in _MERGED:
        _MERGED[name] = _solve(name).merge_regions(outputs=OUTPUTS[name])
    return _MERGED[name]


def _slack(ef, row_off, region, pts):
    """min over the rows of region[i] of (f - E theta) / |E| at pts[i] (unit-row depth inside the region; -inf for region -1)"""
    out = numpy.full(len(pts), -numpy.inf)
    ok = numpy.flatnonzero(region >= 0)
    if not len(ok):
        return out
    r = region[ok]
    cnt = (row_off[r + 1] - row_off[r]).astype(numpy.int64)
    start = numpy.repeat(row_off[r] - numpy.concatenate([[0], numpy.cumsum(cnt)[:-1]]), cnt) + numpy.arange(int(cnt.sum()))
    rows = ef[start]
    P = numpy.repeat(pts[ok], cnt, axis=0)
    s = (rows[:, 0] - numpy.einsum('ij,ij->i', rows[:, 1:], P)) / numpy.linalg.norm(rows[:, 1:], axis=1)
    out[ok] = numpy.minimum.reduceat(s, numpy.concatenate([[0], numpy.cumsum(cnt)[:-1]]))
    return out


def _points(sol, rng, n=100_000):
    """uniform points over the regions' facet centres' box and beyond, plus points at +-{0.5, 1.01} 1e-5 from facet centres"""
    ef, row_off, _ = sol._stacked()
    n_t = ef.shape[1] - 1
    centre, _, status = _lib.facet_centres(ef, row_off)
    ok = (status == 0) & numpy.all(numpy.isfinite(centre), axis=1)
    c = centre[ok]
    lo, hi = c.min(axis=0), c.max(axis=0)
    span = numpy.maximum(hi - lo, 1e-3)
    E = ef[ok, 1:]
    nrm = numpy.linalg.norm(E, axis=1, keepdims=True)
    pick = rng.integers(0, len(c), size=n // 2)
    k = rng.choice([-1.01, -0.5, 0.5, 1.01], size=(n // 2, 1)) * 1e-5
    return numpy.vstack([rng.uniform(lo - 0.2 * span, hi + 0.2 * span, size=(n // 2, n_t)), c[pick] + k * E[pick] / nrm[pick]])


def test_overlapping_solved_program_is_refused():
    src = _solve('c2x20')
    assert src.is_overlapping
    with pytest.raises(ValueError, match='overlapping'):
        src.merge_regions(outputs=[10])
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    import bench
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        c3 = solve_mpqp(bench.build_program('c3'), mpqp_algorithm.graph)
    assert c3.is_overlapping
    with pytest.raises(ValueError, match='overlapping'):
        c3.merge_regions(outputs=[0, 1])


@pytest.mark.parametrize('name', ['c3_l4', 'c3_graph', 'random'])
def test_merged_solution_gives_the_source_answer(name):
    src = _solve(name)
    merged = _merged(name)
    n_t = src.theta_dim()
    n_x = numpy.asarray(src.critical_regions[0].A).reshape(-1, n_t).shape[0]
    outs = list(range(n_x)) if OUTPUTS[name] is None else OUTPUTS[name]
    # partition and laws
    members = merged.merge_info['members']
    assert sorted(i for m in members for i in m) == list(range(len(src)))
    assert [min(m) for m in members] == sorted(min(m) for m in members)
    for r in merged.critical_regions:
        assert isinstance(r, MergedRegion)
        law = numpy.hstack([r.A, r.b])
        for i in r.members:
            s = src.critical_regions[i]
            other = numpy.hstack([numpy.asarray(s.A).reshape(-1, n_t)[outs], numpy.asarray(s.b).reshape(-1, 1)[outs]])
            first = numpy.hstack([numpy.asarray(src.critical_regions[r.members[0]].A).reshape(-1, n_t)[outs],
                                  numpy.asarray(src.critical_regions[r.members[0]].b).reshape(-1, 1)[outs]])
            numpy.testing.assert_array_equal(law, first)
            assert numpy.all(numpy.abs(other - first) <= 2 * TOL * (1.0 + numpy.max(numpy.abs(first))))
    assert merged.is_overlapping is False and merged.is_complete == src.is_complete
    assert merged.point_location_tolerance == src.point_location_tolerance and merged.program is src.program
    # location: where the source's region holds the point twice the location tolerance deep, the merged region holding it has that
    # region as a member and gives the source's x[outputs]; where no source region is within three tolerances, no merged region is
    rng = numpy.random.default_rng(17)
    pts = _points(src, rng)
    tol_loc = src.point_location_tolerance
    x_s, r_s = src.evaluate_batch(pts)
    x_m, r_m = merged.evaluate_batch(pts)
    ef, row_off, _ = src._stacked()
    deep = _slack(ef, row_off, r_s, pts) >= 2 * tol_loc
    assert deep.sum() > 1000
    assert numpy.all(r_m[deep] >= 0)
    owner = numpy.empty(len(src), dtype=numpy.int64)
    for k, m in enumerate(members):
        owner[m] = k
    assert numpy.array_equal(owner[r_s[deep]], r_m[deep])
    want = x_s[deep][:, outs]
    assert numpy.all(numpy.abs(x_m[deep] - want) <= 1e-9 * (1.0 + numpy.abs(want)))
    far = src.locator().query(pts, 3 * tol_loc, False, want_x=False)[0] < 0
    assert far.sum() > 100
    assert numpy.all(r_m[far] < 0)


def _member_rows(src, i):
    r = src.critical_regions[i]
    return numpy.asarray(r.E, float), numpy.asarray(r.f, float).reshape(-1)


@pytest.mark.parametrize('name', ['c3_l4', 'c3_graph'])
def test_members_and_merged_regions_contain_each_other(name):
    src = _solve(name)
    merged = _merged(name)
    multi = [k for k, r in enumerate(merged.critical_regions) if len(r.members) > 1]
    assert multi
    regs = [merged.critical_regions[k] for k in multi]
    pts = hit_and_run_batch([Polytope(r.E, r.f.reshape(-1)) for r in regs], chains=16, samples=4, seed=3)     # [P, 16, 4, n]
    centres, radii = src.chebyshev_centres()
    for k, r in enumerate(regs):
        P = pts[k].reshape(-1, pts.shape[-1])
        inside_some = numpy.zeros(len(P), dtype=bool)
        for i in r.members:
            E, f = _member_rows(src, i)
            inside_some |= numpy.all((P @ E.T - f) / numpy.linalg.norm(E, axis=1) <= 1e-6, axis=1)
        assert inside_some.all(), (name, multi[k], int((~inside_some).sum()))
        for i in r.members:
            if not radii[i] > 1e-8:
                continue
            E, f = _member_rows(src, i)
            Q = hit_and_run_batch(Polytope(E, f), chains=8, samples=2, seed=5).reshape(-1, E.shape[1])
            Q = numpy.vstack([Q, centres[i]])
            assert numpy.all(Q @ r.E.T - r.f.reshape(-1) <= TOL * numpy.maximum(1.0, numpy.abs(r.f.reshape(-1)))), (name, i)


def test_merged_regions_of_the_complete_c3_are_exact_unions():
    """Every merged region of the complete c3 with more than one member against the union of its members by the difference recursion
    (tests/merge_exact_reference.py): no piece fatter than 10 tol outside the members, none of a member outside the region; and
    Solution.compare(merged, source) finds every such member inside its region, with HiGHS's radius.
    The bound is the 10 tol of the generated cases.  By the rule one merge leaves at most a sliver of radius tol max(1, |o|) / 2 (a
    valid row lets the partner stick out that far) plus t* <= tol, 4.75e-8 with |o| <= 7.51 on c3; measured: nothing outside, and at
    most 1.82e-8 of a member missing (regions of up to 4 members), a factor 5 under the bound."""
    src = _solve('c3_graph')
    merged = _merged('c3_graph')
    multi = [k for k, r in enumerate(merged.critical_regions) if len(r.members) > 1]
    assert len(multi) > 200
    worst = (0.0, 0.0)
    for k in multi:
        r = merged.critical_regions[k]
        out, miss = exact.union_defect((r.E, r.f), [_member_rows(src, i) for i in r.members], TOL)
        worst = (max(worst[0], out), max(worst[1], miss))
        assert out <= 10 * TOL and miss <= 10 * TOL, (k, r.members, out, miss)
    print('largest outside, missing:', worst)
    g = merged.compare(src, outputs=OUTPUTS['c3_graph'])
    assert g.wide == 0
    own = numpy.flatnonzero(numpy.isin(g.i, multi))
    found = {(int(g.i[n]), int(g.j[n])): int(n) for n in own}
    for k in multi:
        r = merged.critical_regions[k]
        for i in r.members:
            E, f = _member_rows(src, i)
            want = exact.chebyshev_radius(numpy.vstack([r.E, E]), numpy.concatenate([r.f.reshape(-1), f]))
            if want > 2 * TOL:
                n = found[(k, i)]
                assert g.meets[n] and abs(g.radius[n] - want) <= 1e-9 * (1.0 + want), (k, i, g.radius[n], want)


def test_areas_maximality_and_rows():
    src = _solve('c3_l4')
    merged = _merged('c3_l4')
    assert len(merged) < len(src)
    # areas from slice_2d through the Chebyshev centre of the largest merged region: unchanged in total, and each merged area the sum
    # of its members'
    centres, radii = merged.chebyshev_centres()
    fixed = centres[int(numpy.nanargmax(numpy.where(numpy.isfinite(radii), radii, -1.0)))]
    a_src = src.slice_2d(dims=(0, 1), fixed=fixed).areas
    a_m = merged.slice_2d(dims=(0, 1), fixed=fixed).areas
    assert a_m.sum() > 0.0
    assert abs(a_m.sum() - a_src.sum()) <= 1e-9 * a_src.sum()
    for k, r in enumerate(merged.critical_regions):
        assert abs(a_m[k] - a_src[r.members].sum()) <= 1e-9 * max(1.0, a_src.sum())
    # pairwise maximal: the reference rejects every pair of same-law result regions
    # (pairs whose boxes do not touch cannot share a facet)
    laws = [numpy.hstack([r.A, r.b]).ravel() for r in merged.critical_regions]
    n_t = src.theta_dim()
    boxes = [ref._box(ref._unit(r.E, r.f, n_t)[0], n_t) for r in merged.critical_regions]
    for a, b in itertools.combinations(range(len(merged)), 2):
        if numpy.all(numpy.abs(laws[a] - laws[b]) <= TOL * (1.0 + numpy.max(numpy.abs(laws[a])))) and ref._touch(boxes[a], boxes[b], TOL):
            ra, rb = merged.critical_regions[a], merged.critical_regions[b]
            assert ref.pair_rejected((ra.E, ra.f), (rb.E, rb.f)), (a, b)
    # no redundant rows: every merged row is a facet (LP with the row relaxed by 1)
    for r in merged.critical_regions:
        if len(r.members) == 1:
            continue
        E, f = r.E, r.f.reshape(-1)
        for i in range(len(E)):
            A = E.copy()
            b = f.copy()
            b[i] += 1.0
            lp = linprog(-E[i], A_ub=A, b_ub=b, bounds=[(None, None)] * E.shape[1], method='highs')
            assert lp.status == 3 or -lp.fun > f[i] + 1e-9, 'a redundant row in a merged region'


def test_merge_is_deterministic():
    src = _solve('c3_l4')
    a = src.merge_regions(outputs=[0, 1])
    b = src.merge_regions(outputs=[0, 1])
    assert [r.members for r in a.critical_regions] == [r.members for r in b.critical_regions]
    for x, y in zip(a.critical_regions, b.critical_regions):
        assert numpy.array_equal(x.E, y.E) and numpy.array_equal(x.f, y.f)


def test_search_tree_of_a_merged_solution():
    merged = _merged('c3_l4')
    tree = merged.search_tree()
    pts = _points(merged, numpy.random.default_rng(23), 40_000)
    for inclusive in (False, True):
        assert numpy.array_equal(tree.locate_batch(pts, inclusive=inclusive), merged.get_region_batch(pts, inclusive=inclusive))


def test_library_refuses_bad_arguments():
    rows = numpy.array([[1.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    with pytest.raises(_lib.MpcError, match='unit normals'):
        _lib.merge_regions([0, 2], rows * 2.0)
    big = numpy.tile([[1.0, 1.0, 0.0]], (257, 1))
    with pytest.raises(_lib.MpcError, match='256 rows'):
        _lib.merge_regions([0, 257], big)
    xs, box, st, _ = _lib.merge_regions([0, 2], rows)
    with pytest.raises(_lib.MpcError, match='out of range'):
        _lib.merge_pairs([0, 2], rows, xs, box, [0], [0], TOL)
