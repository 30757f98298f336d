"""Solution.reach_cells on the device against hand cases, the recorded CPU reference of forward_reference.py, the composition
of the existing calls and replayed trajectories; the shapes where the kernels can go wrong, determinism, the library's refusals."""
import warnings

import numpy
import pytest

import exit_cases as xc
import forward_cases as fc
import forward_reference as fref
import invariant_cases as ic
from ppopt_amd import _lib, exit_sets as ex, invariant_set as inv, reach, transition as tr
from ppopt_amd.geometry.polytope import Polytope
from ppopt_amd.geometry.reduce import reduce_rows_of

pytestmark = pytest.mark.gpu

TOL = fc.TOL
BAND = 1e-6              # points this close to a decision are left out
BAND_SHARE = 0.01


def _run(polys, Phi, phi, succ, cells0=None, point=None, **kw):
    """cells0: [(region, rows)], None: the polytopes themselves"""
    n_t = polys[0].shape[1] - 1
    off, ef = xc.csr(polys)
    if cells0 is None:
        cells0 = list(enumerate(polys))
    if cells0:
        coff, crow = xc.csr([r for _, r in cells0])
    else:
        coff, crow = numpy.zeros(1, dtype=numpy.int64), numpy.zeros((0, n_t + 1))
    kw.setdefault('tol', TOL)
    return reach.forward_cells(off, ef, Phi, phi, n_t, succ, coff, crow, [i for i, _ in cells0], cell_point=point, **kw)


def _close(got, want):
    return got.shape == want.shape and bool(numpy.all(numpy.abs(got - want) <= 1e-9 * (1.0 + numpy.abs(want))))


def _lineages(got):
    out = []
    for c in range(len(got)):
        out.append((c,) if got.parent[c] < 0 else out[int(got.parent[c])] + (int(got.region[c]),))
    return out


# ---- 1. the tent map ---------------------------------------------------------------------------------------------------------------------
def test_tent_map_is_exact_through_step_8():
    """forward_cases.tent_cells and tent_rows: step k has the 2^(k + 1) dyadic intervals of length 2^-(k + 1) in order of lineage, G =
    +-2^k, dyadic g; rows, G and g are exact in binary and compared with ==.  Step 8: 512 cells of radius 2^-10.  Every item is a cell
    after 1 + 4 LPs; the two rows of Q go first as redundant, the pulled-back pair is alone then and each of their runs is unbounded
    (in 1-D nothing else bounds the side beyond a reversed row): 2 wide runs per item, and no wide cell."""
    polys, Phi, phi, succ = fc.tent_map()
    steps = 8
    got = _run(polys, Phi, phi, succ, max_steps=steps)
    want = fc.tent_cells(steps)
    n_items = len(want) - 2
    print(got.stats)
    assert got.status == 'DONE' and got.steps == steps and len(got) == len(want) and got.stats['cells_per_step'] == [2 ** (k + 1) for k in range(steps + 1)]
    assert got.rows_of(0).tobytes() == polys[0].tobytes() and got.rows_of(1).tobytes() == polys[1].tobytes()
    iv = xc.intervals([(got.region[c], got.rows_of(c)) for c in range(len(got))])
    for c, w in enumerate(want):
        lo, hi, G, g, region, parent = w
        assert iv[c] == (region, lo, hi) and got.G[c, 0, 0] == G and got.g[c, 0] == g and got.parent[c] == parent, (c, w)
        assert got.step[c] == (0 if parent < 0 else got.step[parent] + 1) and lo <= got.point[c, 0] <= hi
        if parent >= 0:              # where a radius run ended above tol: interior (a point of step 0 is any feasible point)
            assert numpy.array_equal(got.rows_of(c), fc.tent_rows(w)) and lo < got.point[c, 0] < hi, (c, w)
    assert not got.wide.any()
    s = got.stats
    assert (s['items'], s['cells'], s['empty'], s['lps'], s['wide']) == (n_items, n_items, 0, 5 * n_items, 2 * n_items)
    # every initial state follows the tent map through its cell
    th = numpy.random.default_rng(0).uniform(0.0, 1.0, (2000, 1))
    x = th.copy()
    for k in range(steps + 1):
        c = got.locate(th, k)
        assert (c >= 0).all() and numpy.array_equal(got.state_at(th, k), x) and numpy.array_equal(got.region[c] == 0, x[:, 0] <= 0.5)
        x = numpy.where(x <= 0.5, 2.0 * x, 2.0 - 2.0 * x)


# ---- 2. the rotation grid ----------------------------------------------------------------------------------------------------------------
def test_rotation_grid_areas_and_maps():
    """invariant_cases.rotation_grid: the states that leave at the first step are the four corner triangles |t1| + |t2| > s, s = sqrt 2 /
    0.9, of area (2 - s)^2 / 2 each; nothing leaves later (after a step the state lies in the image of the box, {|t1| + |t2| <= 0.9 sqrt 2
    = 1.273}, and 1.273 < s = 1.571), so every step >= 1 keeps 4 - 2 (2 - s)^2.  Every map is (0.9 Rot 45 deg)^k."""
    polys, Phi, phi, succ = ic.rotation_grid()
    got = _run(polys, Phi, phi, succ, max_steps=4)
    v = got.volumes()
    s = numpy.sqrt(2.0) / 0.9
    print(got.stats, v.per_step)
    assert got.status == 'DONE' and got.steps == 4 and not got.wide.any()
    assert abs(v.per_step[0] - 4.0) <= 1e-9 and numpy.all(numpy.abs(v.per_step[1:] - (4.0 - 2.0 * (2.0 - s) ** 2)) <= 1e-9)
    corner, inner = [0, 3, 12, 15], [i for i in range(16) if i not in (0, 3, 12, 15)]
    assert numpy.all(numpy.abs(v.per_root[corner, 1:] - (0.25 - (2.0 - s) ** 2 / 2.0)) <= 1e-9) and numpy.all(numpy.abs(v.per_root[inner] - 0.25) <= 1e-9)
    M = numpy.eye(2)
    for k in range(5):
        at = got.cells_at(k)
        assert numpy.all(numpy.abs(got.G[at] - M) <= 1e-14) and not got.g[at].any()
        M = Phi[0] @ M


def test_rotation_grid_from_a_small_square():
    """initial = [-0.1, 0.1]^2: four cells of area 0.01 at step 0 (the square meets the four inner regions); nothing ever leaves, the area
    stays 0.04, and the images at step k are the pieces of the square scaled by 0.9^k and turned by 45 k degrees"""
    polys, Phi, phi, succ = ic.rotation_grid()
    off, ef = xc.csr(polys)
    coff, crow, creg, cpt = reach.initial_cells(off, ef, 2, [xc.box_rows([-0.1, -0.1], [0.1, 0.1])], TOL)
    assert creg.tolist() == [5, 6, 9, 10]
    got = reach.forward_cells(off, ef, Phi, phi, 2, succ, coff, crow, creg, cell_point=cpt, tol=TOL, max_steps=4)
    v = got.volumes()
    assert got.status == 'DONE' and numpy.all(numpy.abs(v.per_step - 0.04) <= 1e-9)
    a = 0.9 / numpy.sqrt(2.0)
    Rk = numpy.eye(2)
    corners = numpy.array([[-0.1, -0.1], [0.1, -0.1], [-0.1, 0.1], [0.1, 0.1]])
    for k in range(5):
        vs = got.image_vertices(k)
        assert all(x is not None for x in vs)
        back = numpy.vstack(vs) @ numpy.linalg.inv(Rk).T
        assert numpy.all(numpy.abs(back) <= 0.1 + 1e-9)
        assert all(numpy.min(numpy.max(numpy.abs(back - c), axis=1)) <= 1e-9 for c in corners)
        H = got.images(k)
        for rows, x in zip(H, vs):                                   # the H-representation holds its own vertices, tightly
            slack = rows[:, :1] - rows[:, 1:] @ x.T
            assert slack.min() >= -1e-9 and numpy.all(slack.min(axis=1) <= 1e-9)
        Rk = numpy.array([[a, -a], [a, a]]) @ Rk


# ---- 3. against the backward side --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['one_d', 'grid_shift'])
def test_volume_kept_is_what_the_invariant_set_has_not_lost(name):
    """the regions do not overlap: the cells of step k are the states still inside after k steps, so their volume is the volume of the
    regions minus what InvariantSet.volumes() reports lost at the steps before"""
    polys, Phi, phi, succ = xc.one_d_loop(4) if name == 'one_d' else xc.grid_shift()
    n_t = polys[0].shape[1] - 1
    off, ef = xc.csr(polys)
    es = ex.exit_pieces(off, ef, Phi, phi, n_t, succ, tol=TOL)
    back = inv.backward_exit_cells(off, ef, Phi, phi, n_t, ic.predecessors_of(succ), es.piece_off, es.piece_rows, es.source, tol=TOL)
    lost = back.volumes().lost_per_step
    steps = 5
    got = _run(polys, Phi, phi, succ, max_steps=steps)
    kept = got.volumes().per_step
    total = 1.5 if name == 'one_d' else 9.0
    assert back.converged or len(lost) >= steps
    lost = numpy.concatenate([lost, numpy.zeros(steps)])             # converged: nothing leaves after its last step
    want = total - numpy.concatenate([[0.0], numpy.cumsum(lost)])[:steps + 1]
    print(name, got.status, got.stats['cells_per_step'], kept, want)
    assert got.steps == steps and numpy.all(numpy.abs(kept - want) <= 1e-9)
    if name == 'grid_shift':
        assert numpy.all(numpy.abs(kept - (9.0 - 1.5 * numpy.arange(steps + 1))) <= 1e-9)


# ---- 4. against the recorded reference ---------------------------------------------------------------------------------------------------
_IDS = [f'n{c[0]}' for c in fc.SETS]
_CACHE = {}


def _set(case):
    """the set, the recorded reference run (tests/golden, written by forward_reference.py) and the device run from the same step 0:
    loaded and computed once, shared, never modified"""
    if case not in _CACHE:
        polys, Phi, phi = xc.synthetic_set(*case)
        z = numpy.load(fref.golden_path(case))
        succ = [z['succ_idx'][z['succ_off'][i]:z['succ_off'][i + 1]].tolist() for i in range(len(polys))]
        want = fref.unpack(z)
        got = _run(polys, Phi, phi, succ, tol=fc.SET_TOL, max_steps=fc.SET_STEPS)
        _CACHE[case] = (polys, Phi, phi, succ, want, got)
    return _CACHE[case]


@pytest.mark.parametrize('case', fc.SETS, ids=_IDS)
def test_synthetic_sets_against_the_reference(case):
    """knife items with these seeds (the reference alone, run on the CPU, 3 steps, tol = 1e-6): 0 of 3293, 0 of 670, 0 of 89"""
    polys, Phi, phi, succ, (cells, items, status), got = _set(case)
    s = got.stats
    n_knife = sum(i['knife'] for i in items)
    print(f'n_t = {case[0]}: {len(polys)} polytopes; reference {len(items)} items, {n_knife} knife, {len(cells)} cells; device: {len(got)} cells '
          f'{s["cells_per_step"]}, {s["items"]} items, {s["lps"]} LPs, {s["pivots"] / max(1, s["lps"]):.2f} pivots per LP, {s["wide"]} wide runs, '
          f'step ms {s["step_ms"]}, wall {s["wall_ms"]:.1f} ms, status {got.status}')
    assert n_knife <= fc.KNIFE_CAP * len(items)
    lin_got = _lineages(got)
    mine = dict(zip(lin_got, range(len(got))))
    theirs = {c['lineage']: c for c in cells}
    knife = {cells[i['parent']]['lineage'] + (i['region'],) for i in items if i['knife']}      # exempt, with everything that descends from them
    tainted = lambda lin: any(lin[:k] in knife for k in range(2, len(lin) + 1))
    for lin, c in theirs.items():
        if tainted(lin):
            continue
        assert lin in mine, lin
        k = mine[lin]
        assert got.region[k] == c['region'] and got.step[k] == c['step'] and _close(got.rows_of(k), c['rows']), lin
        assert got.G[k].tobytes() == numpy.ascontiguousarray(c['G']).tobytes() and got.g[k].tobytes() == numpy.ascontiguousarray(c['g']).tobytes(), lin
        assert (got.parent[k] < 0 and c['parent'] < 0) or lin_got[int(got.parent[k])] == cells[c['parent']]['lineage']
    assert all(lin in theirs or tainted(lin) for lin in mine)
    if n_knife == 0:         # nothing is exempt: the same cells in the same order, the same counters
        assert [c['lineage'] for c in cells] == lin_got and got.parent.tolist() == [c['parent'] for c in cells] and got.status == status
        assert got.wide.tolist() == [c['wide'] for c in cells]
        assert (s['items'], s['cells'], s['empty']) == (len(items), len(cells) - len(polys), sum(i['outcome'] == 'empty' for i in items))
        # (not the wide runs: a device run stops once t > tol, mostly before it could find that nothing bounds it, and keeps the row
        # either way; the reference's runs go to the end and count every unbounded one)
        assert s['lps'] == sum(i['lps'] for i in items)
    assert len(cells) > len(polys)


# ---- 7. against the composition of the existing calls --------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', fc.SETS, ids=_IDS)
def test_synthetic_sets_against_the_composition(case):
    """per step: transition_pairs over the parents and the regions with the parents' next maps gives the item statuses; reduce_rows_of on
    the parent's rows and pulled_back_rows, started at the parent's point, gives the cell's rows"""
    polys, Phi, phi, succ, _, got = _set(case)
    n_t, R, tol = case[0], len(polys), fc.SET_TOL
    lin = _lineages(got)
    for k in range(1, got.steps + 1):
        parents = numpy.flatnonzero(got.step == k - 1)
        P = numpy.einsum('kab,kbc->kac', Phi[got.region[parents]], got.G[parents])
        p = numpy.einsum('kab,kb->ka', Phi[got.region[parents]], got.g[parents]) + phi[got.region[parents]]
        pa = [n for n, c in enumerate(parents) for _ in succ[got.region[c]]]
        pb = [len(parents) + j for c in parents for j in succ[got.region[c]]]
        aoff, aef = xc.csr([got.rows_of(c) for c in parents] + polys)
        res = tr.transition_pairs(aoff, aef, numpy.concatenate([P, numpy.tile(numpy.eye(n_t), (R, 1, 1))]), numpy.concatenate([p, numpy.zeros((R, n_t))]),
                                  n_t, tol=tol, pairs=(pa, pb))
        edge = {(int(parents[i]), int(j - len(parents))) for i, j, st in zip(res['i'], res['j'], res['status']) if st != tr.NO_EDGE}
        at = numpy.flatnonzero(got.step == k)
        mine = {(int(got.parent[c]), int(got.region[c])) for c in at}
        assert edge == mine, (k, sorted(edge ^ mine))
        where = {int(c): n for n, c in enumerate(parents)}
        rows = []
        for c in at:
            n = where[int(got.parent[c])]
            assert numpy.array_equal(P[n], got.G[c]) or numpy.allclose(P[n], got.G[c], rtol=0, atol=1e-13)
            back = ex.pulled_back_rows(polys[got.region[c]], got.G[c], got.g[c])
            rows.append(numpy.vstack([got.rows_of(got.parent[c]), back[~numpy.isnan(back[:, 0])]]))
        roff, rrows = xc.csr(rows)
        red = reduce_rows_of(roff, rrows, n_t, tol=tol, start=got.point[got.parent[at]])
        assert numpy.all(red.status == 0)
        for n, c in enumerate(at):
            assert _close(got.rows_of(c), red.rows[red.row_off[n]:red.row_off[n + 1]]), (k, lin[c])


# ---- 5. sheared grid partitions: points -------------------------------------------------------------------------------------------------
_GRIDS = {}


def _grid(case):
    """the partition, the device run, 20,000 uniform points of X_0 and their replay: computed once, shared, never modified"""
    if case not in _GRIDS:
        n, g, seed, steps = case
        polys, Phi, phi, succ, M = fc.sheared_grid(n, g, seed)
        got = _run(polys, Phi, phi, succ, tol=fc.SET_TOL, max_steps=steps)
        th = fc.grid_points(M, 20000, 100 + seed)
        _GRIDS[case] = (polys, Phi, phi, M, got, th, fref.replay(polys, Phi, phi, th, steps))
    return _GRIDS[case]


@pytest.mark.parametrize('case', fc.GRIDS, ids=[f'n{c[0]}' for c in fc.GRIDS])
def test_sampled_points_follow_their_cells(case):
    """measured on one MI355X: the largest |state_at - replay| / (1 + |replay|) is recorded in DESIGN §3.25; the bound 1e-9 leaves three
    orders above the rounding of <= 4 steps with |Phi| <= 2 and n_theta <= 3 (below 1e-13)"""
    polys, Phi, phi, M, got, th, (theta, region, near) = _grid(case)
    n, g, seed, steps = case
    assert max(numpy.linalg.norm(P, 2) for P in Phi) <= 2.0 and got.steps == steps and not got.wide.any()
    keep = near > BAND
    vol = got.volumes().per_step
    worst = 0.0
    print(f'n_t = {n}: {len(polys)} regions, cells per step {got.stats["cells_per_step"]}, rows per cell <= {int(numpy.diff(got.cell_off).max())}, '
          f'{got.stats["items"]} items, {got.stats["lps"]} LPs, step ms {got.stats["step_ms"]}; {int((~keep).sum())} of {len(th)} points left out')
    assert int((~keep).sum()) <= BAND_SHARE * len(th)
    for k in range(steps + 1):
        c = got.locate(th, k)
        inside = region[k] >= 0
        assert numpy.array_equal((c >= 0)[keep], inside[keep]), k
        ok = keep & inside
        assert numpy.array_equal(got.region[c[ok]], region[k][ok]) and numpy.all(got.step[c[ok]] == k)
        x = got.state_at(th, k)
        err = numpy.abs(x[ok] - theta[k][ok]) / (1.0 + numpy.abs(theta[k][ok]))
        worst = max(worst, float(err.max()) if err.size else 0.0)
        assert numpy.all(err <= 1e-9) and numpy.all(numpy.isnan(x[keep & ~inside]))
        # the volume kept is the share of the points still inside, within three standard errors of the sample (the binomial's, at the
        # share the volumes state)
        share, N = vol[k] / vol[0], int(keep.sum())
        assert abs(inside[keep].mean() - share) <= 3.0 * numpy.sqrt(share * (1.0 - share) / N) + 1e-12, (k, inside[keep].mean(), share)
    print(f'    largest relative error of state_at: {worst:.3e}; volume kept per step {vol / vol[0]}')
    assert abs(vol[0] - 2.0 ** n * abs(numpy.linalg.det(M))) <= 1e-9


# ---- 6. entering --------------------------------------------------------------------------------------------------------------------------
def test_entering_a_target_first_at_step_2():
    """on the 2-D grid of test 5, the bundle that starts in one region (a target inside X_0 holds initial states of the whole of X_0, so
    the whole has no target that is entered first at step 2): a box around a replayed state of step 2 of that bundle, with no replayed
    state of its steps 0 and 1 within 0.01 of the box, is entered first at step 2; a box far outside X_0 and every image never is.  The
    first region and the first state with such a box are taken; on the CPU the reference's cells enter that box at step 2 alone."""
    case = fc.GRIDS[0]
    polys, Phi, phi, M, _, th, (theta, region, near) = _grid(case)
    succ = [list(range(len(polys))) for _ in polys]
    found = None
    for r0 in range(len(polys)):
        bundle = region[0] == r0
        early = numpy.vstack([theta[0][bundle], theta[1][bundle & (region[1] >= 0)]])
        for centre in theta[2][bundle & (region[2] >= 0)][:50]:
            for half in (0.05, 0.02, 0.01):
                if found is None and not numpy.any(numpy.all(numpy.abs(early - centre) <= half + 0.01, axis=1)):
                    found = (r0, centre, half)
        if found:
            break
    assert found is not None
    r0, centre, half = found
    bundle = region[0] == r0
    got = _run(polys, Phi, phi, succ, cells0=[(r0, polys[r0])], tol=fc.SET_TOL, max_steps=case[3])
    alive2 = bundle & (region[2] >= 0)
    th, theta, near = th[bundle], theta[:, bundle], near[bundle]
    alive2 = alive2[bundle]
    target = xc.box_rows(centre - half, centre + half)
    far = xc.box_rows([50.0, 50.0], [51.0, 51.0])
    hit = got.entering([target, Polytope(far[:, 1:], far[:, :1])], tol=fc.SET_TOL)
    arrive = numpy.all(numpy.abs(theta[2] - centre) <= half, axis=1) & alive2
    print(f'target {centre} +- {half}: first steps {hit.first_step}, {len(hit.cell)} pairs, {int(arrive.sum())} sampled points arrive at step 2')
    assert hit.first_step.tolist() == [2, -1] and len(hit.cells_of(1)) == 0 and arrive.sum() >= 1
    cells2 = set(hit.cells_of(0)[got.step[hit.cells_of(0)] == 2].tolist())
    # every sampled point that arrives at step 2 (away from a decision) sits in a cell that hits
    c = got.locate(th, 2)
    deep = arrive & (near > BAND) & numpy.all(numpy.abs(theta[2] - centre) <= half - BAND, axis=1)
    assert deep.sum() >= 1 and all(int(k) in cells2 for k in c[deep])
    for w, k, t in zip(hit.witness, hit.cell, hit.target):          # a witness is an initial state of its cell whose state lies in the target
        assert t == 0 and numpy.all(got.rows_of(k)[:, 1:] @ w <= got.rows_of(k)[:, 0] + 1e-9)
        assert numpy.all(numpy.abs(got.G[k] @ w + got.g[k] - centre) <= half + 1e-9)


# ---- 8. shapes where the kernels can go wrong ------------------------------------------------------------------------------------------
def test_a_cell_and_a_region_of_256_rows_each():
    """exit_cases.tangent_pair: the cell 'polytope 0, whole' against region 1: 512 rows in LDS at n_theta = 16, 78,840 bytes of rows and
    state, above the 48 KB a kernel gets without the attribute.  The image of polytope 0 lies deep inside polytope 1: the child is polytope
    0 with its own 256 rows and none of the pulled-back ones, after 1 + 512 LPs; region 1 has no successor, so the next step has no item."""
    polys, Phi, phi, succ = xc.tangent_pair()
    got = _run(polys, Phi, phi, succ, cells0=[(0, polys[0])], max_steps=3)
    print(got.stats)
    assert got.status == 'EMPTY' and got.steps == 1 and len(got) == 2 and got.region.tolist() == [0, 1] and got.parent.tolist() == [-1, 0]
    assert got.stats['items'] == 1 and got.stats['lps'] == 513 and not got.wide.any()
    assert got.rows_of(1).tobytes() == polys[0].tobytes()
    P, s = fref.next_map(Phi[0], phi[0], numpy.eye(16), numpy.zeros(16))
    assert got.G[1].tobytes() == P.tobytes() and got.g[1].tobytes() == s.tobytes()


@pytest.mark.parametrize('m_a', [63, 64, 65])
@pytest.mark.parametrize('m_b', [1, 64])
@pytest.mark.parametrize('swapped', [False, True], ids=['cell_first', 'roles_swapped'])
def test_row_counts_across_the_mask_words(m_a, m_b, swapped):
    """invariant_cases.straddle gives a square of m_a rows (4 and redundant tangents) and a half plane x >= 1/2 of m_b rows (1 and
    redundant tangents).  Cell = the square (region 0, theta+ = theta / 2 + (1/4, 0)) against region 1 = the half plane: the child is
    [1/2, 1] x [-1, 1] from the rows 0, 1, 3 of the cell and slot m_a, the first pulled-back row.  Roles swapped: cell = the half plane
    (region 0, theta+ = theta) against region 1 = the square: the same set from row 0 of the cell and the slots m_b + 0, 1, 3."""
    (square,), _, _, ((_, half),) = ic.straddle(m_a, m_b)
    x_ge_half = numpy.array([[-0.5, -1.0, 0.0]])
    if not swapped:
        polys, Phi, phi = [square, half], numpy.stack([0.5 * numpy.eye(2), numpy.eye(2)]), numpy.array([[0.25, 0.0], [0.0, 0.0]])
        want = numpy.vstack([square[[0, 1, 3]], x_ge_half])
        exact = slice(0, 3)
    else:
        polys, Phi, phi = [half, square], numpy.stack([numpy.eye(2), numpy.eye(2)]), numpy.zeros((2, 2))
        want = numpy.vstack([x_ge_half, square[[0, 1, 3]]])
        exact = slice(0, 4)                                          # the identity pulls the axis rows back exactly (a -0.0 comes back as 0.0)
    got = _run(polys, Phi, phi, [[1], []], cells0=[(0, polys[0])], point=[[0.75, 0.0]], max_steps=1)
    assert got.status == 'DONE' and got.steps == 1 and len(got) == 2 and got.region.tolist() == [0, 1]
    assert _close(got.rows_of(1), want) and numpy.array_equal(got.rows_of(1)[exact], want[exact])
    assert got.stats['lps'] == 1 + m_a + m_b and numpy.all(got.rows_of(1)[:, 1:] @ got.point[1] < got.rows_of(1)[:, 0])
    assert got.point[0].tolist() == [0.75, 0.0]


def test_constant_rows_and_a_zero_map():
    """the two cases of tests/test_forward_cpu.py::test_reference_on_constant_rows_and_a_zero_map on the device: empty without an LP,
    dropped rows, and under Phi = 0 the child is the parent whole with G = 0"""
    polys, Phi, phi, succ = xc.constant_rows()
    got = _run(polys, Phi, phi, succ, max_steps=3)
    s = got.stats
    assert got.status == 'EMPTY' and got.steps == 1 and got.step.tolist() == [0, 0, 1] and got.parent.tolist() == [-1, -1, 0] and got.region[2] == 1
    assert [s[k] for k in ('items', 'empty', 'cells', 'lps')] == [5, 4, 1, 7] and not got.wide.any()
    assert numpy.array_equal(got.rows_of(2), numpy.array([[1.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 1.0, 0.0], [0.0, -1.0, 0.0]]))
    assert numpy.array_equal(got.G[2], Phi[0]) and numpy.array_equal(got.g[2], phi[0])
    S = xc.box_rows([0, 0], [1, 1])
    got = _run([S], numpy.zeros((1, 2, 2)), numpy.array([[0.5, 0.5]]), [[0]], max_steps=3)
    assert got.status == 'DONE' and len(got) == 4 and got.stats['lps'] == 15 and got.parent.tolist() == [-1, 0, 1, 2]
    for c in range(1, 4):
        assert got.rows_of(c).tobytes() == S.tobytes() and not got.G[c].any() and got.g[c].tolist() == [0.5, 0.5]
    assert got.image_vertices(2)[0].tolist() == [[0.5, 0.5]] * 4 and got.images(2) == [None]


def test_a_reduced_cell_above_256_rows_is_the_rows_status():
    """a regular 200-gon under the identity against the 200-gon turned by half a side: the child is a 400-gon, every row of it essential
    (a corner it cuts off is about 9e-5 deep, far above tol): 400 > 256 rows, the call stops with status ROWS and returns step 0"""
    polys = [fc.polygon(200), fc.polygon(200, 0.5)]
    got = _run(polys, numpy.tile(numpy.eye(2), (2, 1, 1)), numpy.zeros((2, 2)), [[1], []], cells0=[(0, polys[0])])
    assert got.status == 'ROWS' and got.steps == 0 and len(got) == 1 and got.stats['cells'] == 1 and got.stats['items'] == 1
    assert got.rows_of(0).tobytes() == polys[0].tobytes() and numpy.array_equal(got.G[0], numpy.eye(2))


def test_limits_of_steps_cells_and_rows():
    polys, Phi, phi, succ = fc.tent_map()
    full = _run(polys, Phi, phi, succ, max_steps=4)
    for max_steps in (0, 1, 3):
        got = _run(polys, Phi, phi, succ, max_steps=max_steps)
        assert got.status == 'DONE' and got.steps == max_steps and len(got) == 2 ** (max_steps + 2) - 2
        assert got.cell_rows.tobytes() == full.cell_rows[:full.cell_off[len(got)]].tobytes() and got.G.tobytes() == full.G[:len(got)].tobytes()
    got = _run(polys, Phi, phi, succ, max_cells=10)                  # 2 + 4, step 2 would make 14
    assert got.status == 'MAX_CELLS' and got.steps == 1 and len(got) == 6
    got = _run(polys, Phi, phi, succ, max_rows_total=20)             # 2 rows per cell
    assert got.status == 'MAX_ROWS_TOTAL' and got.steps == 1 and len(got) == 6 and got.stats['cells'] == 12
    none = _run(polys, Phi, phi, succ, cells0=[])
    assert len(none) == 0 and none.status == 'EMPTY' and none.steps == 0
    gone = _run(polys, Phi, phi, [[], []])                           # no region follows: every trajectory has left
    assert len(gone) == 2 and gone.status == 'EMPTY' and gone.steps == 0 and gone.stats['items'] == 0
    with pytest.raises(ValueError, match='step 0'):
        _run(polys, Phi, phi, succ, max_cells=1)


def test_two_runs_give_identical_bits():
    polys, Phi, phi, succ, _, got = _set(fc.SETS[1])
    again = _run(polys, Phi, phi, succ, tol=fc.SET_TOL, max_steps=fc.SET_STEPS)
    for name in ('cell_off', 'cell_rows', 'region', 'step', 'parent', 'wide', 'point', 'G', 'g'):
        assert getattr(again, name).tobytes() == getattr(got, name).tobytes(), name
    keys = ('items', 'cells', 'empty', 'lps', 'pivots', 'wide', 'cells_per_step')
    assert {k: again.stats[k] for k in keys} == {k: got.stats[k] for k in keys} and again.steps == got.steps


def test_solution_form_graph_passed_or_built_and_initial_sets():
    import test_gpu_exit_sets as tx
    sol, plant, graph, _ = tx._case('c2')
    before = [(r.E.copy(), r.f.copy()) for r in sol.critical_regions]
    args = (plant['A'], plant['B'], plant['inputs'])
    got = sol.reach_cells(*args, graph=graph, steps=3)
    built = sol.reach_cells(*args, steps=3)
    for name in ('cell_off', 'cell_rows', 'region', 'step', 'parent', 'wide', 'point', 'G', 'g'):
        assert getattr(built, name).tobytes() == getattr(got, name).tobytes(), name
    assert all(numpy.array_equal(r.E, E) and numpy.array_equal(r.f, f) for r, (E, f) in zip(sol.critical_regions, before))
    assert got.n_regions == len(sol) and numpy.array_equal(got.region[got.step == 0], numpy.arange(len(sol))) and got.steps >= 1
    # the cells agree with a simulated bundle: where a point is located at step k, the simulation is in that region
    polys, Phi, phi = tx._arrays(sol, plant)
    centre = got.point[0]
    small = Polytope(numpy.vstack([numpy.eye(len(centre)), -numpy.eye(len(centre))]), numpy.concatenate([centre + 0.01, -(centre - 0.01)]).reshape(-1, 1))
    part = sol.reach_cells(*args, initial=small, graph=graph, steps=3)
    whole = sol.reach_cells(*args, initial=[small], steps=3)
    assert part.cell_rows.tobytes() == whole.cell_rows.tobytes() and len(part.cells_at(0)) >= 1
    th = centre + numpy.random.default_rng(3).uniform(-0.01, 0.01, (500, len(centre)))
    theta, region, near = fref.replay(polys, Phi, phi, th, part.steps)
    for k in range(part.steps + 1):
        c = part.locate(th, k)
        ok = (near > BAND) & (region[k] >= 0)
        assert numpy.all(c[ok] >= 0) and numpy.array_equal(part.region[c[ok]], region[k][ok])
        assert numpy.all(numpy.abs(part.state_at(th, k)[ok] - theta[k][ok]) <= 1e-9 * (1.0 + numpy.abs(theta[k][ok])))
    with pytest.raises(ValueError, match='steps'):
        sol.reach_cells(*args, steps=-1)
    with pytest.raises(ValueError, match='initial'):
        sol.reach_cells(*args, initial=[])


def test_an_overlapping_source_is_refused():
    from ppopt_amd import problem_generator as pg
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        lp = solve_mpqp(pg.generate_mplp(4, 2, 10, seed=0), mpqp_algorithm.combinatorial)
    A, B = numpy.eye(2), numpy.zeros((2, 1))
    with pytest.raises(ValueError, match='remove_overlaps'):
        lp.reach_cells(A, B, [0])
    red = lp.remove_overlaps()
    stay = red.reach_cells(A, B, [0], steps=2)                           # theta+ = theta: every region maps onto itself, nothing leaves
    assert stay.status == 'DONE' and stay.steps == 2 and len(stay.cells_at(0)) == len(red) and min(stay.stats['cells_per_step']) >= len(red)
    assert numpy.all(numpy.abs(stay.G - numpy.eye(2)) <= 1e-12) and not stay.g.any()
    own = [c for c in stay.cells_at(2) if stay.itinerary(c) == [stay.region[c]] * 3]
    assert sorted(stay.region[own].tolist()) == list(range(len(red)))
    out = red.reach_cells(A, B, [0], c=numpy.array([1000.0, 0.0]), steps=2)   # every state leaves at once: no region has a successor
    assert out.status == 'EMPTY' and out.steps == 0 and out.stats['items'] == 0


def test_library_refusals():
    """MPC_ERR_INVALID (MpcError with the library's message) before any launch"""
    sq = xc.box_rows(numpy.zeros(2), numpy.ones(2))
    off, ef = xc.csr([sq, sq + numpy.array([0.5, 0, 0])])
    Phi, phi = numpy.tile(0.5 * numpy.eye(2), (2, 1, 1)), numpy.zeros((2, 2))
    base = dict(off=off, ef=ef, Phi=Phi, phi=phi, soff=[0, 1, 2], sidx=[1, 0], coff=[0, 4], crow=sq, creg=[0], cpt=[[0.5, 0.5]], tol=TOL, max_steps=2,
                max_cells=8, max_rows=64)
    call = lambda **kw: (lambda a: _lib.forward_cells(a['off'], a['ef'], a['Phi'], a['phi'], a['soff'], a['sidx'], a['coff'], a['crow'], a['creg'], a['cpt'],
                                                      a['tol'], a['max_steps'], a['max_cells'], a['max_rows']))(dict(base, **kw))
    r = call()
    assert r['status'] in range(5) and len(r['region']) >= 1 and r['step'][0] == 0 and numpy.array_equal(r['G'][0], numpy.eye(2))
    assert call(coff=[0], crow=numpy.zeros((0, 3)), creg=[], cpt=numpy.zeros((0, 2)))['status'] == _lib.FORWARD_EMPTY
    nan = ef.copy()
    nan[1, 1] = numpy.nan
    for kw, text in (({'tol': -1.0}, 'tol'), ({'tol': numpy.nan}, 'tol'), ({'ef': nan}, 'finite'), ({'crow': sq * 2.0}, 'unit'),
                     ({'Phi': numpy.full_like(Phi, numpy.inf)}, 'Phi must be finite'), ({'phi': phi + numpy.nan}, 'must be finite'),
                     ({'cpt': [[numpy.nan, 0.5]]}, 'cell_point0 must be finite'), ({'sidx': [1, 2]}, 'out of range'), ({'sidx': [-1, 0]}, 'out of range'),
                     ({'creg': [2]}, 'out of range'), ({'max_steps': -1}, 'max_steps'), ({'off': [0, 0, 8]}, '1..256 rows'),
                     ({'coff': [0, 0, 4], 'creg': [0, 0], 'cpt': numpy.full((2, 2), 0.5)}, '1..256 rows'), ({'soff': [0, 2, 1], 'sidx': [0]}, 'succ_off'),
                     ({'max_cells': 0}, 'step 0')):
        with pytest.raises(_lib.MpcError, match=text):
            call(**kw)
