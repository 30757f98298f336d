"""Solution.transition_graph on the device: the pair stage against the independent CPU reference on an analytic 1-D loop
and on seeded synthetic polytopes with contracting, rotating, rank-deficient, zero and identity maps up to n_theta = 16 and 512 rows
per pair; the box screen loses no edge; the early stop gives the same edges; witnesses; determinism; the solved programs c2 and c3
with their plants, against the reference and against simulated trajectories; merged and reduced solutions."""
import warnings

import numpy
import pytest

import transition_reference as ref
from ppopt_amd import MPQP_Program, _lib, invariance, problem_generator as pg, transition as tr
from ppopt_amd.geometry.polytope import Polytope
from ppopt_amd.geometry.polytope_operations import hit_and_run_batch
from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
from ppopt_amd.region_merge import solution_rows

pytestmark = pytest.mark.gpu

TOL = 1e-8
KNIFE_SHARE = 0.02       # of a set's pairs


def _csr(polys):
    return numpy.concatenate([[0], numpy.cumsum([len(p) for p in polys])]).astype(numpy.int64), numpy.vstack(polys)


def _box_rows(lo, hi):
    n = len(lo)
    return numpy.vstack([numpy.column_stack([hi, numpy.eye(n)]), numpy.column_stack([-lo, -numpy.eye(n)])])


def _compare(pairs, radius, status, want):
    """statuses equal and radii within 1e-9 (1 + |r|), infinities exactly, for every pair the reference does not call knife; returns the
    number of knife pairs"""
    knife = 0
    for k, pair in enumerate(pairs):
        w_status, w_r, w_knife = want[pair]
        if w_knife:
            knife += 1
            continue
        assert tr.STATUS[status[k]] == w_status, (pair, tr.STATUS[status[k]], radius[k], w_status, w_r)
        if numpy.isinf(w_r):
            assert radius[k] == w_r, (pair, radius[k], w_r)
        else:
            assert abs(radius[k] - w_r) <= 1e-9 * (1.0 + abs(w_r)), (pair, radius[k], w_r)
    return knife


def _witnesses_hold(polys, Phi, phi, res):
    """every edge's witness lies in R_i and its image in R_j, within 1e-9 on the rows as given"""
    n = 0
    for k in numpy.flatnonzero((res['status'] == tr.EDGE) | (res['status'] == tr.UNBOUNDED)):
        i, j, th = int(res['i'][k]), int(res['j'][k]), res['witness'][k]
        assert numpy.all(polys[i][:, 1:] @ th <= polys[i][:, 0] + 1e-9), (i, j)
        assert numpy.all(polys[j][:, 1:] @ (Phi[i] @ th + phi[i]) <= polys[j][:, 0] + 1e-9), (i, j)
        n += 1
    return n


# ---- 1. the 1-D loop ---------------------------------------------------------------------------------------------------------------------
def _one_d(a, c_max, T=10.0):
    """min u^2 s.t. |u| <= 1, |a theta + u| <= c_max, |theta| <= T: the plant theta+ = a theta + u"""
    A = numpy.array([[1.0], [-1.0], [1.0], [-1.0]])
    b = numpy.array([[1.0], [1.0], [c_max], [c_max]])
    F = numpy.array([[0.0], [0.0], [-a], [a]])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        prog = MPQP_Program(A, b, numpy.zeros((1, 1)), numpy.zeros((1, 1)), numpy.array([[2.0]]), numpy.array([[1.0], [-1.0]]),
                            numpy.array([[T], [T]]), F)
        sol = solve_mpqp(prog, mpqp_algorithm.combinatorial)
    return _unflagged(sol), numpy.array([[a]]), numpy.array([[1.0]])


def _unflagged(sol):
    """solve_mpqp flags every solution it returns as overlapping, as the reference does; the regions of a strictly convex mpQP do not
    overlap, and transition_graph refuses by the flag: the same program and regions without it"""
    if not sol.is_overlapping:
        return sol
    from ppopt_amd import Solution
    assert numpy.linalg.eigvalsh(sol.program.Q).min() > 0
    plain = Solution(sol.program, sol.critical_regions, is_overlapping=False, point_location_tolerance=sol.point_location_tolerance)
    plain.is_complete = sol.is_complete
    return plain


def _arrays(sol, plant):
    """(unit-row polytopes, Phi, phi) of a solution under its plant, assembled here from the regions and laws"""
    n_t = sol.theta_dim()
    off, rows, _ = solution_rows(sol.critical_regions, n_t, 'test')
    polys = numpy.split(rows, off[1:-1])
    _, _, xlaw = sol._stacked()
    Phi, phi = invariance.closed_loop_maps(xlaw, numpy.asarray(plant['A'], dtype=float), numpy.asarray(plant['B'], dtype=float).reshape(n_t, -1),
                                           numpy.asarray(plant['inputs']))
    return polys, Phi, phi


def test_one_d_all_nine_pairs():
    sol, A, B = _one_d(2.0, 0.5)
    assert len(sol) == 3
    polys, Phi, phi = _arrays(sol, {'A': A, 'B': B, 'inputs': [0]})
    off, ef = _csr(polys)
    pa, pb = numpy.divmod(numpy.arange(9), 3)
    res = tr.transition_pairs(off, ef, Phi, phi, 1, tol=TOL, full_radius=True, pairs=(pa, pb))
    want = ref.graph_reference(polys, Phi, phi, TOL)
    assert _compare(list(zip(res['i'].tolist(), res['j'].tolist())), res['radius'], res['status'], want) == 0
    assert sorted(numpy.round(res['radius'][res['status'] == tr.EDGE], 12).tolist()) == [0.0625, 0.0625, 0.125, 0.25, 0.25]
    assert numpy.sum(res['radius'] == -numpy.inf) == 4 and res['stats']['lps'] == 5
    assert _witnesses_hold(polys, Phi, phi, res) == 5
    g = sol.transition_graph(A, B, [0], full_radius=True)
    assert g.n_regions == 3 and len(g.indices) == 5 and numpy.all(g.status == tr.EDGE) and numpy.all(g.region_status == 0)
    mid = int(numpy.argmax(numpy.diff(g.indptr)))
    assert g.successors(mid).tolist() == [0, 1, 2] and all(g.successors(i).tolist() == [i] for i in range(3) if i != mid)


# ---- 2. synthetic sets -------------------------------------------------------------------------------------------------------------------
KINDS = ('contraction', 'rotation', 'rank_deficient', 'zero', 'identity')


def _map(kind, n, act, rng):
    if kind == 'contraction':
        return 0.5 * numpy.eye(n) + 0.1 * rng.normal(size=(n, n)), rng.uniform(-0.3, 0.3, n)
    if kind == 'rotation':
        q, r = numpy.linalg.qr(rng.normal(size=(n, n)))
        return q * numpy.sign(numpy.diag(r)), numpy.zeros(n)
    if kind == 'rank_deficient':      # one zero singular direction: a zero row, so the target rows along it are constant
        P = 0.5 * rng.normal(size=(n, n))
        P[int(rng.integers(0, act))] = 0.0
        return P, rng.uniform(-0.6, 0.6, n)
    if kind == 'zero':
        return numpy.zeros((n, n)), rng.uniform(-0.6, 0.6, n)
    return numpy.eye(n), numpy.zeros(n)


def synthetic_set(n, seed, k, act=3, size=(0.25, 0.45), balls=0):
    """k polytopes in [-1, 1]^n (a box around a centre that varies in the first ``act`` coordinates, cut by one to three random rows;
    with ``balls``: that many rows tangent to a ball of radius 0.2 instead), then one unbounded region: the cone theta >= c cut by the
    half-space sum theta >= sum c + 0.2 sqrt n, whose map is the identity, so that its self loop is unbounded.  The maps of the others
    go round KINDS."""
    rng = numpy.random.default_rng(seed)
    act = min(n, act)
    polys, Phi, phi = [], [], []
    for q in range(k):
        c, s = numpy.zeros(n), numpy.ones(n)
        c[:act], s[:act] = rng.uniform(-0.5, 0.5, act), rng.uniform(size[0], size[1], act)
        if balls:
            N = rng.normal(size=(balls, n))
            N /= numpy.linalg.norm(N, axis=1, keepdims=True)
            polys.append(numpy.column_stack([N @ c + 0.2, N]))
        else:
            m = int(rng.integers(1, 4))
            N = rng.normal(size=(m, n))
            N /= numpy.linalg.norm(N, axis=1, keepdims=True)
            polys.append(numpy.vstack([_box_rows(c - s, c + s), numpy.column_stack([N @ c + rng.uniform(0.1, 0.3, m), N])]))
        P, p = _map(KINDS[q % len(KINDS)], n, act, rng)
        Phi.append(P)
        phi.append(p)
    if not balls:
        c = rng.uniform(-0.5, 0.0, n)
        one = numpy.ones(n) / numpy.sqrt(n)
        polys.append(numpy.vstack([numpy.column_stack([-c, -numpy.eye(n)]), numpy.append(-(one @ c + 0.2), -one)[None]]))
        Phi.append(numpy.eye(n))
        phi.append(numpy.zeros(n))
    return polys, numpy.asarray(Phi), numpy.asarray(phi)


# (n_theta, seed, polytopes before the cone, varying coordinates, half-widths, ball rows): 12 to 40 polytopes; six of 256 rows at
# n_theta = 16, where a pair holds 512 rows and the LDS of a wavefront exceeds 48 KB
SETS = [(2, 11, 11, 2, (0.25, 0.45), 0), (3, 12, 23, 3, (0.25, 0.45), 0), (5, 13, 39, 3, (0.25, 0.45), 0), (16, 14, 6, 2, (0.1, 0.2), 256)]
_IDS = [f'n{c[0]}' for c in SETS]
_CACHE = {}


def _set(case):
    """the set, its reference over all pairs, and the dense device run with full radii: computed once, shared, never modified"""
    if case not in _CACHE:
        polys, Phi, phi = synthetic_set(*case)
        R = len(polys)
        want = ref.graph_reference(polys, Phi, phi, TOL)
        off, ef = _csr(polys)
        pa, pb = numpy.divmod(numpy.arange(R * R), R)
        dense = tr.transition_pairs(off, ef, Phi, phi, case[0], tol=TOL, full_radius=True, pairs=(pa, pb))
        _CACHE[case] = (polys, Phi, phi, want, off, ef, dense)
    return _CACHE[case]


@pytest.mark.parametrize('case', SETS, ids=_IDS)
def test_synthetic_sets_against_the_reference(case):
    """knife pairs with these seeds (the reference alone, run on the CPU): 0 of 144, 0 of 576, 0 of 1600, 0 of 36"""
    polys, Phi, phi, want, off, ef, dense = _set(case)
    R = len(polys)
    pairs = list(zip(dense['i'].tolist(), dense['j'].tolist()))
    assert pairs == [(i, j) for i in range(R) for j in range(R)]
    knife = _compare(pairs, dense['radius'], dense['status'], want)
    print(f'n_t = {case[0]}: {R * R} pairs, {knife} knife, {dense["stats"]["edges"]} edges, {dense["stats"]["pivots"]} pivots in {dense["stats"]["lps"]} LPs, '
          f'{dense["stats"]["pair_ms"]:.3f} ms')
    assert knife <= KNIFE_SHARE * R * R
    assert dense['stats']['capped'] == 0 and not numpy.any(dense['status'] == tr.UNDECIDED)
    statuses = {v[0] for v in want.values()}
    assert ref.EDGE in statuses and ref.NO_EDGE in statuses
    if not case[5]:
        assert want[(R - 1, R - 1)][0] == ref.UNBOUNDED and dense['status'][-1] == tr.UNBOUNDED     # the cone onto itself
        assert any(v[1] == -numpy.inf for v in want.values()) and any(v[0] == ref.EDGE and (i % 5) in (2, 3) for (i, _), v in want.items())
    if case[5]:
        assert max(len(p) for p in polys) == 256 and _lib.MERGE_MAX_ROWS == 256


@pytest.mark.parametrize('case', SETS, ids=_IDS)
def test_the_screen_loses_no_edge(case):
    polys, Phi, phi, want, off, ef, dense = _set(case)
    res = tr.transition_pairs(off, ef, Phi, phi, case[0], tol=TOL, full_radius=True)
    cand = {pair: k for k, pair in enumerate(zip(res['i'].tolist(), res['j'].tolist()))}
    assert sorted(cand) == list(cand) and numpy.all(res['region_status'] == 0)
    for pair, (status, r, knife) in want.items():
        if status != ref.NO_EDGE:
            assert pair in cand, (pair, status, r)
    _compare(list(cand), res['radius'], res['status'], want)       # a candidate that is no reference edge comes back NO_EDGE
    print(f'n_t = {case[0]}: {len(cand)} candidates of {len(want)} pairs, {res["stats"]["edges"]} edges')
    assert len(cand) < len(want) or case[5]
    # the image boxes are exact: against the images of the regions' Chebyshev centres and of the witnesses
    box = res['image_box']
    for k in numpy.flatnonzero(dense['status'] == tr.EDGE):
        i = int(dense['i'][k])
        img = Phi[i] @ dense['witness'][k] + phi[i]
        assert numpy.all(img >= box[i, 0] - 1e-9) and numpy.all(img <= box[i, 1] + 1e-9)


@pytest.mark.parametrize('case', SETS, ids=_IDS)
def test_the_early_stop_gives_the_same_edges(case):
    polys, Phi, phi, want, off, ef, dense = _set(case)
    fast = tr.transition_pairs(off, ef, Phi, phi, case[0], tol=TOL, full_radius=False, pairs=(dense['i'], dense['j']))
    numpy.testing.assert_array_equal(fast['status'] != tr.NO_EDGE, dense['status'] != tr.NO_EDGE)
    edge = fast['status'] != tr.NO_EDGE
    r, full = fast['radius'][edge], dense['radius'][edge]
    assert numpy.all(r > TOL)
    with numpy.errstate(invalid='ignore'):
        bound = numpy.where(numpy.isinf(full), numpy.inf, full + 1e-9 * (1.0 + numpy.abs(full)))
    assert numpy.all(r <= bound)
    assert fast['stats']['pivots'] <= dense['stats']['pivots']
    print(f'n_t = {case[0]}: pivots {fast["stats"]["pivots"]} with the early stop, {dense["stats"]["pivots"]} without')
    assert _witnesses_hold(polys, Phi, phi, fast) == int(edge.sum())


@pytest.mark.parametrize('case', SETS, ids=_IDS)
def test_witnesses_of_the_synthetic_sets(case):
    polys, Phi, phi, want, off, ef, dense = _set(case)
    assert _witnesses_hold(polys, Phi, phi, dense) == dense['stats']['edges']
    # with the full radius the witness is a Chebyshev centre: every row of R_i has slack >= r there
    for k in numpy.flatnonzero(dense['status'] == tr.EDGE):
        i = int(dense['i'][k])
        assert numpy.all(polys[i][:, 0] - polys[i][:, 1:] @ dense['witness'][k] >= dense['radius'][k] - 1e-9)


def test_two_runs_give_identical_bits():
    polys, Phi, phi, want, off, ef, dense = _set(SETS[1])
    again = tr.transition_pairs(off, ef, Phi, phi, 3, tol=TOL, full_radius=True, pairs=(dense['i'], dense['j']))
    for name in ('radius', 'status', 'witness'):
        assert again[name].tobytes() == dense[name].tobytes(), name
    a, b = (tr.transition_pairs(off, ef, Phi, phi, 3, tol=TOL) for _ in range(2))
    for name in ('i', 'j', 'radius', 'status', 'witness', 'image_box'):
        assert a[name].tobytes() == b[name].tobytes(), name


# ---- 7. plants -----------------------------------------------------------------------------------------------------------------------------
_SOLVED = {}
SIM_SEED = 7


def _case(name):
    if name not in _SOLVED:
        import bench
        from ppopt_amd.mp_solvers import mpqp_hip_combinatorial
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if name == 'c2':
                sol, plant = solve_mpqp(bench.build_program('c2'), mpqp_algorithm.combinatorial), pg.double_integrator_plant(5)
            elif name == 'c3_l4':
                sol, plant = mpqp_hip_combinatorial.solve(bench.build_program('c3'), max_levels=4), pg.quad_tank_plant()
        sol = _unflagged(sol)
        graph = sol.transition_graph(plant['A'], plant['B'], plant['inputs'])
        _SOLVED[name] = (sol, plant, graph)
    return _SOLVED[name]


def _simulated(name):
    """2,000 trajectories of 50 steps from hit-and-run points of the regions, located by the list scan: (region [n, steps])"""
    key = name + '_sim'
    if key not in _SOLVED:
        sol, plant, _ = _case(name)
        R = len(sol)
        chains = -(-2000 // R)
        polys = [Polytope(r.E, r.f) for r in sol.critical_regions]
        pts = hit_and_run_batch(polys, chains=chains, samples=1, n_steps=50, seed=SIM_SEED)[:, :, 0, :]
        th0 = pts.transpose(1, 0, 2).reshape(-1, pts.shape[-1])[:2000]
        _SOLVED[key] = sol.simulate(th0, 50, plant['A'], plant['B'], plant['inputs'], locate='scan').region
    return _SOLVED[key]


@pytest.mark.parametrize('name', ['c2', 'c3_l4'])
def test_plants_against_the_reference(name):
    sol, plant, g = _case(name)
    R = len(sol)
    assert not numpy.any(g.status == tr.UNDECIDED) and not numpy.any(g.region_status == tr.UNDECIDED), g.stats
    polys, Phi, phi = _arrays(sol, plant)
    edges = set(zip(g.sources().tolist(), g.indices.tolist()))
    if R <= 40:
        pairs = [(i, j) for i in range(R) for j in range(R)]
    else:
        rng = numpy.random.default_rng(5)
        extra = set()
        while len(extra) < 1000:
            pair = (int(rng.integers(0, R)), int(rng.integers(0, R)))
            if pair not in edges:
                extra.add(pair)
        pairs = sorted(edges) + sorted(extra)
    want = ref.graph_reference(polys, Phi, phi, TOL, pairs)
    knife = wrong = 0
    for pair in pairs:
        status, r, kn = want[pair]
        if kn:
            knife += 1
        elif (status != ref.NO_EDGE) != (pair in edges):
            wrong += 1
            print('differs:', pair, status, r)
    print(f'{name}: {R} regions, {len(edges)} edges of {g.stats["candidates"]} candidates, {len(pairs)} pairs compared, {knife} knife; '
          f'box {g.stats["box_ms"]:.3f} ms, pairs {g.stats["pair_ms"]:.3f} ms, sweep {g.stats["sweep_ms"]:.1f} ms, '
          f'{g.stats["pivots"] / max(1, g.stats["lps"]):.2f} pivots per LP')
    assert wrong == 0
    # the early stop reports a lower bound above tol; the reference's radius is the bound it stays under
    at = {pair: k for k, pair in enumerate(zip(g.sources().tolist(), g.indices.tolist()))}
    for pair in edges:
        status, r, kn = want[pair]
        if not kn:
            assert TOL < g.radius[at[pair]] <= r + 1e-9 * (1.0 + abs(r)), (pair, g.radius[at[pair]], r)
    # witnesses
    for k, (i, j) in enumerate(zip(g.sources().tolist(), g.indices.tolist())):
        th = g.witness[k]
        ri, rj = sol.critical_regions[i], sol.critical_regions[j]
        assert numpy.all(ri.E @ th <= ri.f.reshape(-1) + 1e-9), (i, j)
        assert numpy.all(rj.E @ (Phi[i] @ th + phi[i]) <= rj.f.reshape(-1) + 1e-9), (i, j)


@pytest.mark.parametrize('name', ['c2', 'c3_l4'])
def test_plants_simulated_transitions_are_edges(name):
    sol, plant, g = _case(name)
    region = _simulated(name)
    a, b = region[:, :-1].reshape(-1), region[:, 1:].reshape(-1)
    on = (a >= 0) & (b >= 0)
    seen, count = numpy.unique(numpy.stack([a[on], b[on]], axis=1), axis=0, return_counts=True)
    missing = [(int(i), int(j), int(c)) for (i, j), c in zip(seen, count) if not g.has_edge(int(i), int(j))]
    n_missing = sum(c for _, _, c in missing)
    print(f'{name}: {int(on.sum())} observed transitions over {len(seen)} distinct pairs; {len(missing)} pairs ({n_missing} transitions) are no edges')
    if missing:
        polys, Phi, phi = _arrays(sol, plant)
        for i, j, _ in missing:
            status, r, _ = ref.pair_reference(polys[i], polys[j], Phi[i], phi[i], TOL)
            assert r <= TOL + ref.KNIFE, (i, j, status, r)
    assert n_missing <= 1e-3 * int(on.sum())


def test_steps_to_the_origin_on_c2():
    sol, plant, g = _case('c2')
    origin = [i for i, r in enumerate(sol.critical_regions) if numpy.all(r.f.reshape(-1) > 1e-9)]
    assert len(origin) == 1
    t = origin[0]
    assert g.has_edge(t, t) and g.successors(t).tolist() == [t]
    lower, upper = g.steps_to([t])
    region = _simulated('c2')
    checked = 0
    for row in region:
        hit = numpy.flatnonzero(row == t)
        stays = numpy.all(row[:hit[0]] >= 0) if len(hit) else numpy.all(row >= 0)
        if not stays or row[0] < 0:
            continue
        i = int(row[0])
        if len(hit):
            assert lower[i] <= hit[0] <= upper[i], (i, int(hit[0]), lower[i], upper[i])
        else:
            assert upper[i] > len(row) - 1, (i, upper[i])
        checked += 1
    print(f'c2: {checked} trajectories checked; lower up to {numpy.max(lower[numpy.isfinite(lower)])}, finite upper on '
          f'{int(numpy.isfinite(upper).sum())} of {len(upper)} regions; cycles outside the target: {len(g.cycles_outside([t]))}')
    assert checked > 1000


# ---- 8. merged and reduced solutions ---------------------------------------------------------------------------------------------------
def test_a_merged_solution_builds_a_graph():
    sol, plant, _ = _case('c3_l4')
    merged = sol.merge_regions(outputs=[0, 1])
    assert len(merged) < len(sol)
    mp = dict(plant, inputs=[0, 1])
    g = merged.transition_graph(mp['A'], mp['B'], mp['inputs'])
    assert g.n_regions == len(merged) and len(g.indices) > 0
    polys, Phi, phi = _arrays(merged, mp)
    for k, (i, j) in enumerate(zip(g.sources().tolist(), g.indices.tolist())):
        th = g.witness[k]
        ri, rj = merged.critical_regions[i], merged.critical_regions[j]
        assert numpy.all(ri.E @ th <= ri.f.reshape(-1) + 1e-9), (i, j)
        assert numpy.all(rj.E @ (Phi[i] @ th + phi[i]) <= rj.f.reshape(-1) + 1e-9), (i, j)


def test_a_reduced_mplp_is_accepted_and_the_unreduced_one_refused():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sol = solve_mpqp(pg.generate_mplp(4, 2, 10, seed=0), mpqp_algorithm.combinatorial)
    assert sol.is_overlapping
    A, B = numpy.eye(2), numpy.zeros((2, 1))        # theta+ = theta: every region keeps its points, T_ii = R_i
    with pytest.raises(ValueError, match='remove_overlaps'):
        sol.transition_graph(A, B, [0])
    red = sol.remove_overlaps()
    assert not red.is_overlapping and red.overlap_info is not None
    g = red.transition_graph(A, B, [0], full_radius=True)
    assert g.n_regions == len(red) and not numpy.any(g.status == tr.UNDECIDED)
    polys, Phi, phi = _arrays(red, {'A': A, 'B': B, 'inputs': [0]})
    for i in range(len(red)):
        assert g.has_edge(i, i)
        k = int(g.indptr[i] + numpy.searchsorted(g.successors(i), i))
        want = ref.pair_reference(polys[i], polys[i], Phi[i], phi[i], TOL)
        assert want[0] == ref.EDGE and abs(g.radius[k] - want[1]) <= 1e-9 * (1.0 + abs(want[1]))


# ---- the library's refusals -------------------------------------------------------------------------------------------------------------
def test_library_refusals():
    """MPC_ERR_INVALID (MpcError with the library's message) before any launch; a self loop and an empty pair list are fine"""
    sq = _box_rows(numpy.zeros(2), numpy.ones(2))
    off, ef = _csr([sq, sq + numpy.array([0.5, 0, 0])])
    Phi, phi, xs = numpy.tile(numpy.eye(2), (2, 1, 1)), numpy.zeros((2, 2)), numpy.array([[0.5, 0.5], [1.0, 0.5]])
    pairs = lambda **kw: _lib.transition_pairs(kw.get('off', off), kw.get('ef', ef), kw.get('Phi', Phi), kw.get('phi', phi), kw.get('xs', xs),
                                               kw.get('a', [0]), kw.get('b', [0]), True, kw.get('tol', TOL))
    boxes = lambda **kw: _lib.transition_boxes(kw.get('off', off), kw.get('ef', ef), kw.get('Phi', Phi), kw.get('phi', phi), kw.get('xs', xs))
    r, st, w, stats = pairs()
    assert st.tolist() == [tr.EDGE] and abs(r[0] - 0.5) <= 1e-12 and stats['pairs'] == 1
    assert pairs(a=[], b=[])[3]['pairs'] == 0
    box, flag, _ = boxes()
    numpy.testing.assert_allclose(box, [[[0, 0], [1, 1]], [[-0.5, -0.5], [1.5, 1.5]]], atol=1e-12)      # the second square is [-1/2, 3/2]^2
    assert flag.tolist() == [0, 0]
    nan = ef.copy()
    nan[1, 1] = numpy.nan
    for call, kw, text in ((pairs, {'tol': -1.0}, 'tol'), (pairs, {'tol': numpy.nan}, 'tol'), (pairs, {'ef': nan}, 'finite'), (boxes, {'ef': nan}, 'finite'),
                           (pairs, {'Phi': Phi * numpy.inf}, 'Phi must be finite'), (boxes, {'Phi': Phi * numpy.nan}, 'Phi must be finite'),
                           (pairs, {'phi': phi + numpy.nan}, 'finite'), (boxes, {'xs': xs * numpy.inf}, 'finite'), (pairs, {'xs': xs + numpy.nan}, 'finite'),
                           (pairs, {'b': [2]}, 'out of range'), (pairs, {'a': [-1]}, 'out of range'),
                           (pairs, {'off': [0, 0, 8]}, '1..256 rows'), (boxes, {'off': [0, 0, 8]}, '1..256 rows')):
        with pytest.raises(_lib.MpcError, match=text):
            call(**kw)
