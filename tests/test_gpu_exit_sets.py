"""Solution.exit_sets on the device: the hand cases of tests/exit_cases.py; seeded synthetic sets against the independent CPU
reference, up to n_theta = 16 and 512 rows per item; and without the reference: membership of sampled points, the volume identity on
grid partitions, simulated steps on the solved programs c2 and c3; determinism, merged and reduced solutions, the library's refusals."""
import time
import warnings

import numpy
import pytest

import exit_cases as ec
import exit_reference as ref
from ppopt_amd import MPQP_Program, Solution, _lib, exit_sets as ex, invariance, problem_generator as pg, transition as tr
from ppopt_amd.geometry.polytope import Polytope
from ppopt_amd.geometry.polytope_operations import hit_and_run_batch
from ppopt_amd.geometry.volume import volumes_of_rows
from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
from ppopt_amd.region_merge import solution_rows

pytestmark = pytest.mark.gpu

TOL = 1e-8
KNIFE_SHARE = 0.02       # of a case's regions
BAND = 1e-6              # points this close to a decision are left out
BAND_SHARE = 0.01


def _compare(got, want, knife):
    """outside the knife regions: the same pieces in the same order with the same sources, rows within 1e-9 (1 + |value|), none wide"""
    keep = [k for k in range(len(got)) if int(got.source[k]) not in knife]
    want = [p for p in want if p[0] not in knife]
    assert [int(got.source[k]) for k in keep] == [p[0] for p in want], (got.source.tolist(), [p[0] for p in want])
    for k, (src, rows, wide, whole) in zip(keep, want):
        mine = got.rows_of(k)
        assert mine.shape == rows.shape, (k, src, mine.shape, rows.shape)
        assert numpy.all(numpy.abs(mine - rows) <= 1e-9 * (1.0 + numpy.abs(rows))), (k, src, float(numpy.max(numpy.abs(mine - rows))))
        assert not got.wide[k] and not wide
    for i in range(got.n_regions):
        if i not in knife:
            assert bool(got.whole[i]) == any(p[0] == i and p[3] for p in want), i
    assert got.stats['wide'] == 0


def _margin_outside(polys, img):
    """[n]: min over the polytopes of the largest row violation at img: positive iff the point lies in no polytope"""
    out = numpy.full(len(img), numpy.inf)
    for rows in polys:
        out = numpy.minimum(out, numpy.max(img @ rows[:, 1:].T - rows[:, 0], axis=1))
    return out


# ---- 1. the hand cases -----------------------------------------------------------------------------------------------------------------
def _run(case):
    polys, Phi, phi, succ = case
    off, ef = ec.csr(polys)
    return ex.exit_pieces(off, ef, Phi, phi, ef.shape[1] - 1, succ, tol=TOL)


def test_one_d_mismatched_plant_by_hand():
    es = _run(ec.one_d_loop(4))
    got = ec.intervals([(es.source[k], es.rows_of(k)) for k in range(len(es))])
    want = [(0, -0.75, -0.25), (1, 0.1875, 0.25), (1, -0.25, -0.1875), (2, 0.25, 0.75)]
    assert [g[0] for g in got] == [0, 1, 1, 2] and es.whole.tolist() == [True, False, True] and not es.wide.any()
    numpy.testing.assert_allclose(sorted(g[1:] for g in got), sorted(w[1:] for w in want), rtol=0, atol=1e-9)
    assert es.stats['rounds'] == 3 and es.stats['items'] == 1 + 2 + 2 and es.stats['wide'] == 0
    v = es.volumes()
    numpy.testing.assert_allclose(v.exit, [0.5, 0.125, 0.5], rtol=0, atol=1e-12)
    numpy.testing.assert_allclose(v.share, [1.0, 0.25, 1.0], rtol=0, atol=1e-12)
    assert abs(v.exit.sum() - 1.125) <= 1e-12 and abs(v.region.sum() - 1.5) <= 1e-12 and abs(v.total_share - 0.75) <= 1e-12
    assert es.contains([[0.2], [0.1], [-0.5], [0.8]]).tolist()[1::2] == [-1, -1] and (es.contains([[0.2], [-0.5]]) >= 0).all()


def _unflagged(sol):
    """solve_mpqp flags every solution as overlapping; the regions of a strictly convex mpQP do not overlap: the same regions without it"""
    if not sol.is_overlapping:
        return sol
    assert numpy.linalg.eigvalsh(sol.program.Q).min() > 0
    plain = Solution(sol.program, sol.critical_regions, is_overlapping=False, point_location_tolerance=sol.point_location_tolerance)
    plain.is_complete = sol.is_complete
    return plain


def _one_d_solution():
    A = numpy.array([[1.0], [-1.0], [1.0], [-1.0]])
    b = numpy.array([[1.0], [1.0], [0.5], [0.5]])
    F = numpy.array([[0.0], [0.0], [-2.0], [2.0]])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        prog = MPQP_Program(A, b, numpy.zeros((1, 1)), numpy.zeros((1, 1)), numpy.array([[2.0]]), numpy.array([[1.0], [-1.0]]),
                            numpy.array([[10.0], [10.0]]), F)
        return _unflagged(solve_mpqp(prog, mpqp_algorithm.combinatorial))


def test_one_d_solved_program_under_both_plants():
    sol = _one_d_solution()
    assert len(sol) == 3
    es = sol.exit_sets(numpy.array([[4.0]]), numpy.array([[1.0]]), [0])
    got = sorted((lo, hi) for _, lo, hi in ec.intervals([(es.source[k], es.rows_of(k)) for k in range(len(es))]))
    numpy.testing.assert_allclose(got, [(-0.75, -0.25), (-0.25, -0.1875), (0.1875, 0.25), (0.25, 0.75)], rtol=0, atol=1e-9)
    assert int(es.whole.sum()) == 2 and not es.wide.any()
    v = es.volumes()
    assert abs(v.exit.sum() - 1.125) <= 1e-9 and abs(v.region.sum() - 1.5) <= 1e-9
    matched = sol.exit_sets(numpy.array([[2.0]]), numpy.array([[1.0]]), [0])
    assert len(matched) == 0 and not matched.whole.any() and matched.stats['items'] == 5
    assert matched.volumes().exit.tolist() == [0.0, 0.0, 0.0]


def test_grid_and_constant_rows_by_hand():
    es = _run(ec.grid_shift(0.5))
    assert es.source.tolist() == [2, 5, 8] and not es.whole.any() and not es.wide.any()
    v = es.volumes()
    numpy.testing.assert_allclose(v.piece, [0.5, 0.5, 0.5], rtol=0, atol=1e-9)
    for k, r in enumerate(range(3)):
        rows = es.rows_of(k)
        corners = numpy.array([[2.5, r], [3, r], [2.5, r + 1], [3, r + 1]], dtype=float)
        assert numpy.all(corners @ rows[:, 1:].T <= rows[:, 0] + 1e-9)
        assert numpy.all(numpy.isnan(v.share[[3 * r, 3 * r + 1]]) | (v.share[[3 * r, 3 * r + 1]] == 0.0)) and abs(v.share[3 * r + 2] - 0.5) <= 1e-9
    polys, Phi, phi, succ = ec.constant_rows()
    es = _run((polys, Phi, phi, succ))
    assert es.source.tolist() == [1] and es.whole.tolist() == [False, True]
    numpy.testing.assert_array_equal(es.rows_of(0), polys[1])
    assert es.stats['lps'] == 1 + 2          # A against C_AB: the intersection and its two rows with a normal; B's cutters are empty: no LP


# ---- 2. seeded synthetic sets against the reference --------------------------------------------------------------------------------------
_IDS = [f'n{c[0]}' for c in ec.SETS]
_CACHE = {}


def _set(case):
    """the set, the reference's graph and pieces, and the device run: computed once, shared, never modified"""
    if case not in _CACHE:
        polys, Phi, phi = ec.synthetic_set(*case)
        t0 = time.perf_counter()
        succ, graph_knife = ref.successors_reference(polys, Phi, phi, TOL)
        want, knife = ref.exit_reference(polys, Phi, phi, succ, TOL)
        ref_s = time.perf_counter() - t0
        off, ef = ec.csr(polys)
        got = ex.exit_pieces(off, ef, Phi, phi, case[0], succ, tol=TOL)
        _CACHE[case] = (polys, Phi, phi, succ, want, knife | graph_knife, got, off, ef, ref_s)
    return _CACHE[case]


@pytest.mark.parametrize('case', ec.SETS, ids=_IDS)
def test_synthetic_sets_against_the_reference(case):
    """knife regions with these seeds (the reference alone, run on the CPU): 0 of 12, 0 of 24, 0 of 40"""
    polys, Phi, phi, succ, want, knife, got, off, ef, ref_s = _set(case)
    s = got.stats
    print(f'n_t = {case[0]}: {len(polys)} polytopes, {sum(map(len, succ))} edges, {len(knife)} knife regions, {len(want)} reference pieces in {ref_s:.1f} s; '
          f'device: {len(got)} pieces, {s["rounds"]} rounds, {s["items"]} items, {s["lps"]} LPs, {s["pivots"]} pivots, {s["device_ms"]:.3f} ms, '
          f'wall {s["wall_ms"]:.1f} ms')
    assert len(knife) <= KNIFE_SHARE * len(polys)
    _compare(got, want, knife)
    assert len(want) > 0 and any(not p[3] for p in want)


def test_two_polytopes_of_256_rows():
    """an item holds 512 rows at n_theta = 16: 78,840 bytes of LDS, above the 48 KB a kernel gets without the attribute"""
    polys, Phi, phi, succ = ec.tangent_pair()
    assert [len(p) for p in polys] == [256, 256] and _lib.MERGE_MAX_ROWS == 256
    want, knife = ref.exit_reference(polys, Phi, phi, succ, TOL)
    assert not knife and [(p[0], p[3]) for p in want] == [(1, True)]
    es = _run((polys, Phi, phi, succ))
    _compare(es, want, knife)
    assert es.stats['items'] == 1 and es.stats['max_item_rows'] == 512 and es.stats['lps'] == 257


# ---- 3. membership ------------------------------------------------------------------------------------------------------------------------
def _uniform_points(polys, n_points, seed):
    """about n_points points, uniform on every polytope of a synthetic set (its box is its first 2 n rows), and the polytope of each"""
    rng = numpy.random.default_rng(seed)
    n = polys[0].shape[1] - 1
    per = -(-n_points // len(polys))
    pts, reg = [], []
    for i, rows in enumerate(polys):
        hi, lo = rows[:n, 0], -rows[n:2 * n, 0]
        p = numpy.zeros((0, n))
        while len(p) < per:
            cand = rng.uniform(lo, hi, (4 * per, n))
            p = numpy.vstack([p, cand[numpy.all(cand @ rows[:, 1:].T <= rows[:, 0], axis=1)]])
        pts.append(p[:per])
        reg.append(numpy.full(per, i))
    return numpy.vstack(pts)[:n_points], numpy.concatenate(reg)[:n_points]


@pytest.mark.parametrize('case', ec.SETS, ids=_IDS)
def test_membership_of_sampled_points(case):
    polys, Phi, phi, succ, want, knife, got, off, ef, _ = _set(case)
    th, reg = _uniform_points(polys, 20000, seed=100 + case[0])
    img = numpy.einsum('ktl,kl->kt', Phi[reg], th) + phi[reg]
    # a point of several polytopes (they overlap) follows the map of the one it was drawn from; the pieces of that one decide
    margin = _margin_outside(polys, img)
    piece_margin = numpy.full(len(th), numpy.inf)
    for i in range(len(polys)):
        at = numpy.flatnonzero(reg == i)
        ks = got.pieces_of(i)
        for k in ks:
            rows = got.rows_of(k)
            piece_margin[at] = numpy.minimum(piece_margin[at], numpy.max(th[at] @ rows[:, 1:].T - rows[:, 0], axis=1))
    keep = (numpy.abs(margin) > BAND) & (numpy.abs(piece_margin) > BAND)
    wrong = int(numpy.sum(keep & ((piece_margin <= 0.0) != (margin > 0.0))))
    print(f'n_t = {case[0]}: {len(th)} points, {int((~keep).sum())} left out, {int((margin > 0)[keep].sum())} exit, {wrong} disagree')
    assert int((~keep).sum()) <= BAND_SHARE * len(th)
    assert wrong == 0
    assert int((margin > 0)[keep].sum()) > 100 and int((margin <= 0)[keep].sum()) > 100
    hit = got.contains(th)
    assert numpy.all(hit[keep & (piece_margin <= 0.0)] >= 0)


# ---- 4. the volume identity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,cells,seed', [(2, 4, 31), (3, 3, 32)], ids=['2d_4x4', '3d_3x3x3'])
def test_volume_identity_on_a_grid(n, cells, seed):
    """the cells partition the box [0, cells]^n, so R_i is X_i and the T_ij = R_i n C_ij up to boundaries:
    vol(X_i) + sum_j vol(T_ij) = vol(R_i)"""
    rng = numpy.random.default_rng(seed)
    idx = numpy.stack(numpy.meshgrid(*[numpy.arange(cells)] * n, indexing='ij'), axis=-1).reshape(-1, n)
    polys = [ec.box_rows(c, c + 1.0) for c in idx.astype(float)]
    R = len(polys)
    centre = numpy.full(n, cells / 2.0)
    Phi = numpy.stack([0.8 * numpy.eye(n) + 0.25 * rng.normal(size=(n, n)) for _ in range(R)])
    phi = numpy.stack([centre - Phi[i] @ centre + rng.uniform(-0.8, 0.8, n) for i in range(R)])
    off, ef = ec.csr(polys)
    res = tr.transition_pairs(off, ef, Phi, phi, n, tol=TOL)
    edge = res['status'] != tr.NO_EDGE
    assert not numpy.any(res['status'] == tr.UNDECIDED)
    src, dst = res['i'][edge], res['j'][edge]
    succ = [dst[src == i] for i in range(R)]
    es = ex.exit_pieces(off, ef, Phi, phi, n, succ, tol=TOL)
    assert es.stats['wide'] == 0 and len(es) > 0
    v = es.volumes()
    T = [numpy.vstack([polys[i], r[~numpy.isnan(r[:, 0])]]) for i, j in zip(src, dst) for r in [ex.pulled_back_rows(polys[j], Phi[i], phi[i])]]
    toff, trows = ec.csr(T)
    tv = volumes_of_rows(toff, trows, n)
    assert numpy.all(tv.status == _lib.VOL_OK) and numpy.all(v.piece_status == _lib.VOL_OK), (tv.status.tolist(), v.piece_status.tolist())
    stays = numpy.zeros(R)
    numpy.add.at(stays, src, tv.volume)
    worst = float(numpy.max(numpy.abs(v.exit + stays - v.region)))
    print(f'{n}-D grid: {R} cells, {int(edge.sum())} edges, {len(es)} pieces, exit share {v.total_share:.4f}, worst defect {worst:.3e}')
    assert numpy.all(numpy.abs(v.exit + stays - v.region) <= 1e-9 * (1.0 + v.region))
    assert numpy.all(numpy.abs(v.region - 1.0) <= 1e-12) and 0.0 < v.total_share < 1.0


# ---- 5. solved programs -------------------------------------------------------------------------------------------------------------------
_SOLVED = {}
SAMPLE_SEED, SIM_SEED = 5, 7


def _case(name):
    if name not in _SOLVED:
        import bench
        from ppopt_amd.mp_solvers import mpqp_hip_combinatorial
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if name == 'c2':
                sol, plant = solve_mpqp(bench.build_program('c2'), mpqp_algorithm.combinatorial), pg.double_integrator_plant(5)
            else:
                sol, plant = mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4), pg.quad_tank_plant()
        sol = _unflagged(sol)
        graph = sol.transition_graph(plant['A'], plant['B'], plant['inputs'])
        es = sol.exit_sets(plant['A'], plant['B'], plant['inputs'], graph=graph)
        _SOLVED[name] = (sol, plant, graph, es)
    return _SOLVED[name]


def _arrays(sol, plant):
    n_t = sol.theta_dim()
    off, rows, _ = solution_rows(sol.critical_regions, n_t, 'test')
    polys = numpy.split(rows, off[1:-1])
    _, _, xlaw = sol._stacked()
    Phi, phi = invariance.closed_loop_maps(xlaw, numpy.asarray(plant['A'], dtype=float), numpy.asarray(plant['B'], dtype=float).reshape(n_t, -1),
                                           numpy.asarray(plant['inputs']))
    return polys, Phi, phi


@pytest.mark.parametrize('name', ['c2', 'c3_l4'])
def test_plants_against_the_reference_on_a_sample(name):
    """measured on one MI355X with these seeds: config 2, 1 of its 9 regions compared piece by piece and 8 knife regions as sets (no
    reference sliver); four-level config 3, 1 of the 50 sampled regions piece by piece and 49 knife regions as sets (77 reference
    slivers of radius <= 1e-6 among 722 reference pieces); the reference takes 26 to 28 s for the 50 regions"""
    sol, plant, g, es = _case(name)
    R = len(sol)
    polys, Phi, phi = _arrays(sol, plant)
    sample = sorted(numpy.random.default_rng(SAMPLE_SEED).choice(R, size=min(50, R), replace=False).tolist())
    t0 = time.perf_counter()
    want, knife = ref.exit_reference(polys, Phi, phi, [g.successors(i) for i in range(R)], TOL, regions=sample)
    s = es.stats
    print(f'{name}: {R} regions, {len(g.indices)} edges, {len(es)} pieces ({int(es.whole.sum())} regions whole), {s["rounds"]} rounds, {s["items"]} items, '
          f'{s["lps"]} LPs, {s["pivots"] / max(1, s["lps"]):.2f} pivots per LP, device {s["device_ms"]:.3f} ms, wall {s["wall_ms"]:.1f} ms; reference on '
          f'{len(sample)} regions: {len(want)} pieces, {len(knife)} with a knife decision, {time.perf_counter() - t0:.1f} s')
    assert s['wide'] == 0 and not es.wide.any()
    import transition_reference as tref
    exact = thin = 0
    for i in sample:
        mine, theirs = es.pieces_of(i), [p for p in want if p[0] == i]
        if i not in knife:
            exact += 1
            assert len(mine) == len(theirs), (i, len(mine), len(theirs))
            for k, (_, rows, wide, whole) in zip(mine, theirs):
                got = es.rows_of(k)
                assert got.shape == rows.shape and numpy.all(numpy.abs(got - rows) <= 1e-9 * (1.0 + numpy.abs(rows))), (i, k)
            assert bool(es.whole[i]) == any(p[3] for p in theirs)
            continue
        # a knife region: the reference itself does not decide some candidate there (the regions partition the space, so a child and the
        # next cutter share a facet and the candidate behind it has radius exactly 0; HiGHS answers within its own 1e-7), and a candidate
        # decided the other way adds a sliver and a redundant row to the later children.  The pieces then agree as sets up to slivers: each
        # side's pieces of radius above BAND have their Chebyshev centre in a piece of the other side.
        for _, rows, _, _ in theirs:
            _, r, centre = tref.chebyshev(rows)
            if r <= BAND:
                thin += 1
                continue
            assert any(numpy.all(es.rows_of(k)[:, 1:] @ centre <= es.rows_of(k)[:, 0] + 1e-9) for k in mine), (i, r)
        for k in mine:
            _, r, centre = tref.chebyshev(es.rows_of(k))
            assert r > TOL - ref.KNIFE, (i, k, r)
            if r > BAND:
                assert any(numpy.all(rows[:, 1:] @ centre <= rows[:, 0] + 1e-9) for _, rows, _, _ in theirs), (i, k, r)
    print(f'{name}: {exact} sampled regions compared piece by piece, {len(sample) - exact} knife regions compared as sets ({thin} reference slivers)')
    # a region with no successor leaves whole
    none = numpy.flatnonzero(numpy.diff(g.indptr) == 0)
    assert es.whole[none].all() and all(len(es.pieces_of(i)) == 1 for i in none)
    assert numpy.all(numpy.diff(es.source) >= 0) and es.n_regions == R
    if name == 'c3_l4':
        assert len(es) > 0          # the solution is truncated: some images leave it


@pytest.mark.parametrize('name', ['c2', 'c3_l4'])
def test_plants_one_simulated_step(name):
    sol, plant, g, es = _case(name)
    R = len(sol)
    chains = -(-5000 // R)
    pts = hit_and_run_batch([Polytope(r.E, r.f) for r in sol.critical_regions], chains=chains, samples=1, n_steps=50, seed=SIM_SEED)[:, :, 0, :]
    th0 = numpy.ascontiguousarray(pts.transpose(1, 0, 2).reshape(-1, pts.shape[-1])[:5000])
    exact = Solution(sol.program, sol.critical_regions, is_overlapping=False, point_location_tolerance=0.0)
    exact.is_complete = sol.is_complete
    region = exact.simulate(th0, 2, plant['A'], plant['B'], plant['inputs'], locate='scan').region
    polys, Phi, phi = _arrays(sol, plant)
    start = region[:, 0]
    on = start >= 0
    th, start = th0[on], start[on]
    img = numpy.einsum('ktl,kl->kt', Phi[start], th) + phi[start]
    margin = _margin_outside(polys, img)
    piece_margin = numpy.full(len(th), numpy.inf)
    for i in numpy.unique(start):
        at = numpy.flatnonzero(start == i)
        for k in es.pieces_of(i):
            rows = es.rows_of(k)
            piece_margin[at] = numpy.minimum(piece_margin[at], numpy.max(th[at] @ rows[:, 1:].T - rows[:, 0], axis=1))
    # a start on a facet shared by two regions may carry the other one's law: out with the points within BAND of their region's facets
    own = numpy.zeros(len(th))
    for i in numpy.unique(start):
        at = numpy.flatnonzero(start == i)
        own[at] = numpy.max(th[at] @ polys[i][:, 1:].T - polys[i][:, 0], axis=1)
    keep = (numpy.abs(margin) > BAND) & (numpy.abs(piece_margin) > BAND) & (own < -BAND)
    left = region[on, 1] < 0
    hit = es.contains(th) >= 0
    wrong = int(numpy.sum(keep & (left != hit)))
    print(f'{name}: {len(th)} points, {int((~keep).sum())} left out, {int(left[keep].sum())} leave in one step, {wrong} disagree')
    assert int((~keep).sum()) <= BAND_SHARE * len(th)
    assert wrong == 0
    numpy.testing.assert_array_equal(left[keep], margin[keep] > 0.0)


# ---- 6. further checks ------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bits():
    polys, Phi, phi, succ, want, knife, got, off, ef, _ = _set(ec.SETS[1])
    again = ex.exit_pieces(off, ef, Phi, phi, 3, succ, tol=TOL)
    for name in ('piece_off', 'piece_rows', 'source', 'wide', 'whole'):
        assert getattr(again, name).tobytes() == getattr(got, name).tobytes(), name
    assert {k: again.stats[k] for k in ('rounds', 'items', 'lps', 'pivots', 'wide')} == {k: got.stats[k] for k in ('rounds', 'items', 'lps', 'pivots', 'wide')}


def test_graph_passed_in_or_built_inside():
    sol, plant, g, es = _case('c3_l4')
    built = sol.exit_sets(plant['A'], plant['B'], plant['inputs'])
    for name in ('piece_off', 'piece_rows', 'source', 'wide', 'whole'):
        assert getattr(built, name).tobytes() == getattr(es, name).tobytes(), name
    before = [(r.E.copy(), r.f.copy()) for r in sol.critical_regions[:5]]
    sol.exit_sets(plant['A'], plant['B'], plant['inputs'], graph=g)
    assert all(numpy.array_equal(r.E, E) and numpy.array_equal(r.f, f) for r, (E, f) in zip(sol.critical_regions, before))


def test_a_merged_solution_is_accepted():
    sol, plant, _, _ = _case('c3_l4')
    merged = sol.merge_regions(outputs=[0, 1])
    assert len(merged) < len(sol)
    es = merged.exit_sets(plant['A'], plant['B'], [0, 1])
    assert es.n_regions == len(merged) and len(es) > 0 and numpy.all(numpy.diff(es.source) >= 0)
    polys, Phi, phi = _arrays(merged, dict(plant, inputs=[0, 1]))
    # every piece is its region's rows followed by cutting rows, and is not empty
    _, _, status, _ = _lib.merge_regions(es.piece_off, es.piece_rows)
    assert numpy.all(status == 0)
    for k in range(len(es)):
        region = polys[int(es.source[k])]
        numpy.testing.assert_array_equal(es.rows_of(k)[:len(region)], region)


def test_a_reduced_mplp_is_accepted_and_the_unreduced_one_refused():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sol = solve_mpqp(pg.generate_mplp(4, 2, 10, seed=0), mpqp_algorithm.combinatorial)
    assert sol.is_overlapping
    A, B = numpy.eye(2), numpy.zeros((2, 1))
    with pytest.raises(ValueError, match='remove_overlaps'):
        sol.exit_sets(A, B, [0])
    red = sol.remove_overlaps()
    stay = red.exit_sets(A, B, [0])                      # theta+ = theta: nothing leaves
    assert stay.n_regions == len(red) and len(stay) == 0
    out = red.exit_sets(A, B, [0], c=numpy.array([1000.0, 0.0]))      # every image lies far outside: every region leaves whole
    assert len(out) == int(out.whole.sum()) > 0 and not out.wide.any() and out.stats['items'] == 0


def test_library_refusals():
    """MPC_ERR_INVALID (MpcError with the library's message) before any launch; an empty item list is fine"""
    sq = ec.box_rows(numpy.zeros(2), numpy.ones(2))
    off, ef = ec.csr([sq, sq + numpy.array([0.5, 0, 0])])
    Phi, phi = numpy.tile(numpy.eye(2), (2, 1, 1)), numpy.zeros((2, 2))
    call = lambda **kw: _lib.exit_split(kw.get('off', off), kw.get('ef', ef), kw.get('Phi', Phi), kw.get('phi', phi), kw.get('poff', off), kw.get('pef', ef),
                                        kw.get('p', [1]), kw.get('i', [1]), kw.get('j', [0]), kw.get('start', None), kw.get('tol', TOL))
    flag, mask, stats = call()
    assert flag.tolist() == [_lib.OVERLAP_MEETS] and stats['items'] == 1 and stats['meets'] == 1 and mask[0].tolist() == [15, 0, 0, 0]      # [-1/2, 3/2]^2 minus [0, 1]^2: all four rows cut
    assert call(p=[], i=[], j=[])[2]['items'] == 0
    nan = ef.copy()
    nan[1, 1] = numpy.nan
    for kw, text in (({'tol': -1.0}, 'tol'), ({'tol': numpy.nan}, 'tol'), ({'ef': nan}, 'finite'), ({'pef': nan}, 'finite'),
                     ({'Phi': Phi * numpy.inf}, 'Phi must be finite'), ({'phi': phi + numpy.nan}, 'phi must be finite'),
                     ({'start': numpy.array([[numpy.inf, 0.0]])}, 'start must be finite'), ({'j': [2]}, 'out of range'), ({'i': [-1]}, 'out of range'),
                     ({'p': [2]}, 'out of range'), ({'off': [0, 0, 8]}, '1..256 rows'), ({'poff': [0, 0, 8]}, '1..256 rows')):
        with pytest.raises(_lib.MpcError, match=text):
            call(**kw)
