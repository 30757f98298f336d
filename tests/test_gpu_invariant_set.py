"""Solution.invariant_set on the device against hand cases, the CPU reference of invariant_reference.py, the composition of
the existing calls, replayed and simulated trajectories; the shapes where the kernels can go wrong, determinism, the library's refusals."""
import time
import warnings

import numpy
import pytest

import exit_cases as xc
import exit_reference as xref
import invariant_cases as ic
import invariant_reference as iref
from ppopt_amd import Solution, _lib, exit_sets as ex, invariant_set as inv, transition as tr
from ppopt_amd.geometry.polytope import Polytope
from ppopt_amd.geometry.polytope_operations import hit_and_run_batch
from ppopt_amd.geometry.reduce import reduce_rows_of
from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
from ppopt_amd import problem_generator as pg

pytestmark = pytest.mark.gpu

TOL = ic.TOL
BAND = 1e-6              # points this close to a decision are left out
BAND_SHARE = 0.01


def _cells_csr(cells0, n_t):
    if not cells0:
        return numpy.zeros(1, dtype=numpy.int64), numpy.zeros((0, n_t + 1)), numpy.zeros(0, dtype=numpy.int64)
    off, rows = xc.csr([r for _, r in cells0])
    return off, rows, numpy.asarray([s for s, _ in cells0], dtype=numpy.int64)


def _run(polys, Phi, phi, pred, cells0, **kw):
    n_t = polys[0].shape[1] - 1
    off, ef = xc.csr(polys)
    coff, crow, csrc = _cells_csr(cells0, n_t)
    kw.setdefault('tol', TOL)
    return inv.backward_exit_cells(off, ef, Phi, phi, n_t, pred, coff, crow, csrc, **kw)


def _close(got, want):
    return got.shape == want.shape and bool(numpy.all(numpy.abs(got - want) <= 1e-9 * (1.0 + numpy.abs(want))))


def _lineages(got):
    """the name of every cell, whatever the order: its step-0 cell, then the region of every later step"""
    out = []
    for c in range(len(got)):
        out.append((c,) if got.parent[c] < 0 else out[int(got.parent[c])] + (int(got.source[c]),))
    return out


# ---- 1. the 1-D hand case ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tol', [1e-8, 1e-3])
def test_one_d_mismatched_plant_by_hand(tol):
    """invariant_cases.one_d_cells0: per side a large and a small cell per step tile [0.1875 / 4^k, 0.1875 / 4^(k-1)]; a cell is
    reported while its radius exceeds tol, so from the step at which the small cell's radius (1/128) / 4^(k-1) has fallen to tol the large
    cell alone is left, and the part of the interval it misses is thinner than 2 tol."""
    polys, Phi, phi, succ = xc.one_d_loop(4)
    off, ef = xc.csr(polys)
    es = ex.exit_pieces(off, ef, Phi, phi, 1, succ, tol=tol)
    want0 = xc.intervals(ic.one_d_cells0())
    got0 = xc.intervals([(es.source[k], es.rows_of(k)) for k in range(len(es))])
    assert [g[0] for g in got0] == [w[0] for w in want0] and numpy.allclose([g[1:] for g in got0], [w[1:] for w in want0], rtol=0, atol=1e-9)
    got = inv.backward_exit_cells(off, ef, Phi, phi, 1, ic.predecessors_of(succ), es.piece_off, es.piece_rows, es.source, tol=tol)
    steps, small_until = ic.one_d_steps(tol)
    print(f'tol = {tol}: {len(got)} cells, steps {got.steps} (by hand {steps}; small cells until step {small_until}), status {got.status}, stats {got.stats}')
    assert got.converged and got.status == 'CONVERGED' and got.steps == steps and not got.wide.any()
    assert numpy.array_equal(got.step[:4], [0, 0, 0, 0]) and numpy.array_equal(got.parent[:4], [-1] * 4)
    assert got.stats['cells_per_step'] == [4] + [4 if k <= small_until else 2 for k in range(1, steps + 1)]
    iv = xc.intervals([(got.source[c], got.rows_of(c)) for c in range(len(got))])
    for k in range(1, steps + 1):
        at = numpy.flatnonzero(got.step == k)
        assert numpy.all(got.source[at] == 1) and numpy.all(got.step[got.parent[at]] == k - 1) and numpy.all(numpy.diff(got.parent[at]) > 0)
        for c in at:         # the cell is its parent pulled back through theta+ = 4 theta
            assert abs(iv[c][1] - iv[got.parent[c]][1] / 4) <= 1e-9 and abs(iv[c][2] - iv[got.parent[c]][2] / 4) <= 1e-9
        lo, hi = 0.1875 / 4.0 ** k, 0.1875 / 4.0 ** (k - 1)
        for sign in (-1.0, 1.0):
            side = sorted((min(sign * iv[c][1], sign * iv[c][2]), max(sign * iv[c][1], sign * iv[c][2])) for c in at if sign * iv[c][1] > 0)
            assert len(side) == (2 if k <= small_until else 1)
            assert abs(side[-1][1] - hi) <= 1e-9
            if k <= small_until:
                assert abs(side[0][0] - lo) <= 1e-9 and abs(side[0][1] - side[1][0]) <= 1e-9
            else:
                assert 0.0 <= side[0][0] - lo <= 2.0 * tol + 1e-9
    # points: the exit step of theta in M is the first k with 4^k |theta| > 3/4 ... by the cells
    th = numpy.array([[0.5], [0.2], [0.1], [0.02], [0.004], [0.0], [0.8], [-0.06]])
    assert got.exit_step(th).tolist() == [1, 1, 2, 3, 4, 0, -1, 2]
    assert got.contains(th).tolist() == [False, False, False, False, False, True, False, False]


def test_one_d_under_its_own_plant():
    polys, Phi, phi, succ = xc.one_d_loop(2)
    off, ef = xc.csr(polys)
    es = ex.exit_pieces(off, ef, Phi, phi, 1, succ, tol=TOL)
    got = inv.backward_exit_cells(off, ef, Phi, phi, 1, ic.predecessors_of(succ), es.piece_off, es.piece_rows, es.source, tol=TOL)
    assert len(es) == 0 and len(got) == 0 and got.converged and got.steps == 0 and got.stats['items'] == 0
    assert got.exit_step(numpy.array([[0.3], [2.0]])).tolist() == [0, -1]


# ---- 2. the 2-D hand case ----------------------------------------------------------------------------------------------------------------
def test_rotation_grid_by_hand():
    """invariant_cases.rotation_grid: E_0 is the four corner triangles |t1| + |t2| > sqrt 2 / 0.9, step 1 is empty (the docstring there)"""
    polys, Phi, phi, succ = ic.rotation_grid()
    off, ef = xc.csr(polys)
    es = ex.exit_pieces(off, ef, Phi, phi, 2, succ, tol=TOL)
    got = inv.backward_exit_cells(off, ef, Phi, phi, 2, ic.predecessors_of(succ), es.piece_off, es.piece_rows, es.source, tol=TOL)
    # a triangle may come in two pieces, split along the preimage of a grid line
    assert got.converged and got.steps == 0 and sorted(set(got.source.tolist())) == [0, 3, 12, 15] and got.stats['items'] == 16 * len(es) and got.stats['cells'] == 0
    s = numpy.sqrt(2.0) / 0.9
    for corner in [(-1, -1), (1, -1), (-1, 1), (1, 1)]:
        inside = numpy.array(corner) * (1.0 - (2.0 - s) / 3.0) + numpy.array([0.01, 0.02])
        assert got.exit_step(numpy.array([inside, numpy.array(corner) * (s / 2 - 1e-3)])).tolist() == [1, 0]
    v = got.volumes()
    assert numpy.allclose(v.lost_per_region[[0, 3, 12, 15]], (2.0 - s) ** 2 / 2.0, rtol=0, atol=1e-9) and abs(v.share - ic.ROTATION_SHARE) <= 1e-9
    assert abs(v.lost_per_step[0] - 2.0 * (2.0 - s) ** 2) <= 1e-9 and numpy.count_nonzero(v.lost_per_region) == 4
    for reduce_rows in (False, True):
        ps = got.pieces(reduce_rows=reduce_rows)
        pv = ps.volumes()
        assert abs(pv.total_share - ic.ROTATION_SHARE) <= 1e-9 and ps.whole.sum() == 12 and not ps.wide.any()
        assert numpy.all(numpy.diff(ps.source) >= 0) and ps.n_regions == 16


# ---- 3. against the reference ------------------------------------------------------------------------------------------------------------
_IDS = [f'n{c[0]}' for c in ic.SETS]
_CACHE = {}


def _set(case):
    """the set, the reference's graph, exit pieces and cells, and the device run from the same step 0: computed once, shared, never modified"""
    if case not in _CACHE:
        polys, Phi, phi = xc.synthetic_set(*case)
        t0 = time.perf_counter()
        succ, _ = xref.successors_reference(polys, Phi, phi, TOL)
        pieces, _ = xref.exit_reference(polys, Phi, phi, succ, TOL)
        cells0 = [(s, rows) for s, rows, _, _ in pieces]
        pred = ic.predecessors_of(succ)
        want = iref.backward_reference(polys, Phi, phi, pred, cells0, TOL, ic.MAX_STEPS)
        ref_s = time.perf_counter() - t0
        got = _run(polys, Phi, phi, pred, cells0, max_steps=ic.MAX_STEPS)
        _CACHE[case] = (polys, Phi, phi, pred, cells0, want, got, ref_s)
    return _CACHE[case]


@pytest.mark.parametrize('case', ic.SETS, ids=_IDS)
def test_synthetic_sets_against_the_reference(case):
    """knife items with these seeds (the reference alone, run on the CPU, max_steps = 4): 0 of 1113, 0 of 1343, 0 of 473"""
    polys, Phi, phi, pred, cells0, (cells, items, conv), got, ref_s = _set(case)
    s = got.stats
    n_knife = sum(i['knife'] for i in items)
    print(f'n_t = {case[0]}: {len(polys)} polytopes, {len(cells0)} cells at step 0; reference {len(items)} items, {n_knife} knife, {len(cells)} cells in '
          f'{ref_s:.1f} s; device: {len(got)} cells {s["cells_per_step"]}, {s["items"]} items, {s["lps"]} LPs, {s["pivots"] / max(1, s["lps"]):.2f} pivots per LP, '
          f'{s["wide"]} wide runs, step ms {s["step_ms"]}, wall {s["wall_ms"]:.1f} ms, status {got.status}')
    assert n_knife <= ic.KNIFE_CAP * len(items)
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
        assert got.source[k] == c['source'] and got.step[k] == c['step'] and _close(got.rows_of(k), c['rows']), lin
        assert (got.parent[k] < 0 and c['parent'] < 0) or lin_got[int(got.parent[k])] == cells[c['parent']]['lineage']
    assert all(lin in theirs or tainted(lin) for lin in mine)
    if n_knife == 0:         # nothing is exempt: the same cells in the same order
        assert [c['lineage'] for c in cells] == lin_got
        assert got.parent.tolist() == [c['parent'] for c in cells] and got.converged == conv
        assert s['items'] == len(items) and s['cells'] == len(cells) - len(cells0) and s['empty'] == sum(i['outcome'] == 'empty' for i in items)
    assert len(cells) > len(cells0)


# ---- 4. against the composition of the existing calls --------------------------------------------------------------------------------------
def _back(rows, P, p):
    """the pulled-back rows that keep a normal"""
    back = ex.pulled_back_rows(rows, P, p)
    return back[~numpy.isnan(back[:, 0])]


@pytest.mark.parametrize('case', ic.SETS, ids=_IDS)
def test_synthetic_sets_against_the_composition(case):
    """per step: transition_pairs on regions + cells gives the item statuses; reduce_rows_of on the region's rows and pulled_back_rows,
    started where the radius run ended (InvariantSet.point), gives the cell's rows"""
    polys, Phi, phi, pred, cells0, _, got, _ = _set(case)
    n_t, R = case[0], len(polys)
    off, ef = xc.csr(polys)
    lin = _lineages(got)
    for k in range(1, got.steps + 1):
        parents = numpy.flatnonzero(got.step == k - 1)
        pa = [i for c in parents for i in pred[got.source[c]]]
        pb = [R + n for n, c in enumerate(parents) for _ in pred[got.source[c]]]
        aoff, aef = xc.csr(polys + [got.rows_of(c) for c in parents])
        P = numpy.concatenate([Phi, numpy.tile(numpy.eye(n_t), (len(parents), 1, 1))])
        p = numpy.concatenate([phi, numpy.zeros((len(parents), n_t))])
        res = tr.transition_pairs(aoff, aef, P, p, n_t, tol=TOL, pairs=(pa, pb))
        edge = {(int(i), int(parents[j - R])) for i, j, st in zip(res['i'], res['j'], res['status']) if st != tr.NO_EDGE}
        mine = {(int(got.source[c]), int(got.parent[c])) for c in numpy.flatnonzero(got.step == k)}
        assert edge == mine, (k, sorted(edge ^ mine))
        at = numpy.flatnonzero(got.step == k)
        rows = [numpy.vstack([polys[got.source[c]], _back(got.rows_of(got.parent[c]), Phi[got.source[c]], phi[got.source[c]])]) for c in at]
        roff, rrows = xc.csr(rows)
        red = reduce_rows_of(roff, rrows, n_t, tol=TOL, start=got.point[at])
        assert numpy.all(red.status == 0)
        for n, c in enumerate(at):
            assert _close(got.rows_of(c), red.rows[red.row_off[n]:red.row_off[n + 1]]), (k, lin[c])


# ---- 5. without a reference: points -----------------------------------------------------------------------------------------------------
def _uniform_points(polys, n_points, seed):
    """n_points points, uniform on the boxes of the polytopes of a synthetic set (a box is the first 2 n rows), as many per polytope"""
    rng = numpy.random.default_rng(seed)
    n = polys[0].shape[1] - 1
    per = -(-n_points // len(polys))
    return numpy.vstack([rng.uniform(-rows[n:2 * n, 0], rows[:n, 0], (per, n)) for rows in polys])[:n_points]


@pytest.mark.parametrize('case', ic.SETS, ids=_IDS)
def test_exit_step_of_sampled_points_against_a_replay(case):
    """the polytopes of a synthetic set overlap: a state has a trajectory per choice of a polytope that holds it, and a cell holds the
    states some choice takes out, so exit_step is the earliest exit over the choices (invariant_reference.replay_exit_step)"""
    polys, Phi, phi, pred, cells0, _, got, _ = _set(case)
    th = _uniform_points(polys, 20000, 11 + case[0])
    want, near = iref.replay_exit_step(polys, Phi, phi, th, got.steps + 2)
    if not got.converged:
        want = numpy.where(want > got.steps + 1, 0, want)      # cells exist for the exits up to step steps + 1 only
    mine = got.exit_step(th)
    keep = near > BAND
    wrong = int(numpy.sum(keep & (mine != want)))
    print(f'n_t = {case[0]}: {len(th)} points, {int((~keep).sum())} left out, exit steps {numpy.bincount(want[keep] + 1).tolist()} (from -1), {wrong} disagree')
    assert int((~keep).sum()) <= BAND_SHARE * len(th)
    assert wrong == 0
    if got.converged:
        assert not numpy.any(want[keep] > got.steps + 1)
    assert numpy.array_equal(got.contains(th), mine == 0)


def _exact(sol):
    exact = Solution(sol.program, sol.critical_regions, is_overlapping=False, point_location_tolerance=0.0)
    exact.is_complete = sol.is_complete
    return exact


_PLANTS = {}
_MAX_STEPS = {'c2': 6, 'c3_l4': 3}      # the truncated config 3 loses cells for many steps: three bound the test's time


def _plant(name):
    """the solved programs of tests/test_gpu_exit_sets.py (solved once per session there) and their invariant sets"""
    if name not in _PLANTS:
        import test_gpu_exit_sets as tx
        sol, plant, graph, es = tx._case(name)
        got = sol.invariant_set(plant['A'], plant['B'], plant['inputs'], graph=graph, exits=es, max_steps=_MAX_STEPS[name])
        _PLANTS[name] = (sol, plant, graph, es, got, tx._arrays(sol, plant))
    return _PLANTS[name]


@pytest.mark.parametrize('name', ['c2', 'c3_l4'])
def test_plants_simulated_trajectories(name):
    sol, plant, graph, es, got, (polys, Phi, phi) = _plant(name)
    R = len(sol)
    chains = -(-5000 // R)
    pts = hit_and_run_batch([Polytope(r.E, r.f) for r in sol.critical_regions], chains=chains, samples=1, n_steps=50, seed=7)[:, :, 0, :]
    th0 = numpy.ascontiguousarray(pts.transpose(1, 0, 2).reshape(-1, pts.shape[-1])[:5000])
    horizon = got.steps + 2
    region = _exact(sol).simulate(th0, horizon + 1, plant['A'], plant['B'], plant['inputs'], locate='scan').region[:, :horizon + 1]
    out = region < 0
    sim = numpy.where(out.any(axis=1), out.argmax(axis=1), 0)
    sim[out[:, 0]] = -1
    if not got.converged:
        sim = numpy.where(sim > got.steps + 1, 0, sim)
    _, near = iref.replay_exit_step(polys, Phi, phi, th0, horizon)
    mine = got.exit_step(th0)
    in_wide = numpy.zeros(len(th0), dtype=bool)
    for c in numpy.flatnonzero(got.wide):
        in_wide |= numpy.all(th0 @ got.rows_of(c)[:, 1:].T <= got.rows_of(c)[:, 0], axis=1)
    keep = (near > BAND) & ~in_wide
    wrong = int(numpy.sum(keep & (mine != sim)))
    s = got.stats
    print(f'{name}: {R} regions, {len(es)} exit pieces, {len(got)} cells {s["cells_per_step"]}, steps {got.steps}, status {got.status}, {int(got.wide.sum())} wide, '
          f'{s["items"]} items, {s["lps"]} LPs, step ms {s["step_ms"]}, wall {s["wall_ms"]:.1f} ms; {len(th0)} points, {int((~keep).sum())} left out, '
          f'exit steps {numpy.bincount(sim[keep] + 1).tolist()} (from -1), {wrong} disagree')
    assert int((~keep).sum()) <= BAND_SHARE * len(th0)
    assert wrong == 0
    stay = keep & got.contains(th0)
    assert not out[stay][:, :got.steps + 2].any()


# ---- 6. shapes where the kernels can go wrong ------------------------------------------------------------------------------------------
def test_two_polytopes_of_256_rows():
    """region 0 against the cell 'polytope 1, whole': 512 rows in LDS at n_theta = 16, 78,840 bytes, above the 48 KB a kernel gets without
    the attribute.  The image of polytope 0 lies deep inside polytope 1, so the cell is polytope 0 with its own 256 rows and none of the
    pulled-back ones; polytope 0 has no predecessor, so the next step has no item: converged after one step."""
    polys, Phi, phi, succ = xc.tangent_pair()
    got = _run(polys, Phi, phi, ic.predecessors_of(succ), [(1, polys[1])])
    print(got.stats)
    assert got.converged and got.steps == 1 and len(got) == 2 and got.source.tolist() == [1, 0] and got.parent.tolist() == [-1, 0]
    assert got.stats['items'] == 1 and got.stats['lps'] == 513 and not got.wide.any()
    assert got.rows_of(1).tobytes() == polys[0].tobytes()


@pytest.mark.parametrize('m_i', [63, 64, 65])
@pytest.mark.parametrize('m_q', [1, 64])
def test_row_counts_across_the_mask_words(m_i, m_q):
    """invariant_cases.straddle: the cell is [1/2, 1] x [-1, 1] from the rows 0, 1, 3 of the region and slot m_i, the first row of Q"""
    polys, Phi, phi, cells0 = ic.straddle(m_i, m_q)
    got = _run(polys, Phi, phi, [[0]], cells0, max_steps=1)
    assert got.status == 'MAX_STEPS' and not got.converged and got.steps == 1 and len(got) == 2
    want = numpy.vstack([polys[0][[0, 1, 3]], [[-0.5, -1.0, 0.0]]])
    assert _close(got.rows_of(1), want) and got.rows_of(1)[:3].tobytes() == want[:3].tobytes()
    assert got.stats['lps'] == 1 + m_i + m_q and numpy.all(numpy.isfinite(got.point[1])) and numpy.all(numpy.isnan(got.point[0]))
    assert numpy.all(got.rows_of(1)[:, 1:] @ got.point[1] < got.rows_of(1)[:, 0])


def test_constant_rows_of_each_sign():
    """Phi = 0 with theta+ = (1/2, 1/2) on the square S = [0, 1]^2: every pulled-back row is constant.  Against the cell [0, 1] x [0, 3/4]
    every beta is >= 0: the rows are dropped, the new cell is S itself, one LP for the radius and four for its rows.  Against the cell
    [0, 1] x [3/4, 1] the row -y <= -3/4 has beta = -1/4 < -tol: empty, no LP.
    Rank-deficient Phi = diag(1, 0) with the shift (0.1, 1/2): the rows in y are constant with the same two outcomes, the rows in x
    become x <= 0.9 (kept) and -x <= 0.1 (redundant): the cell [0, 0.9] x [0, 1] keeps y <= 1, -x <= 0, -y <= 0 of S and x <= 0.9, after
    1 + 4 + 2 LPs."""
    S = xc.box_rows([0, 0], [1, 1])
    low, high = xc.box_rows([0, 0], [1, 0.75]), xc.box_rows([0, 0.75], [1, 1])
    got = _run([S], numpy.zeros((1, 2, 2)), numpy.array([[0.5, 0.5]]), [[0]], [(0, low), (0, high)], max_steps=1)
    assert got.parent.tolist() == [-1, -1, 0] and [got.stats[k] for k in ('items', 'empty', 'cells', 'lps')] == [2, 1, 1, 5]
    assert got.rows_of(2).tobytes() == S.tobytes() and not got.wide.any()
    got = _run([S], numpy.array([[[1.0, 0.0], [0.0, 0.0]]]), numpy.array([[0.1, 0.5]]), [[0]], [(0, low), (0, high)], max_steps=1)
    assert got.parent.tolist() == [-1, -1, 0] and [got.stats[k] for k in ('items', 'empty', 'cells', 'lps')] == [2, 1, 1, 7]
    assert _close(got.rows_of(2), numpy.vstack([S[[1, 2, 3]], [[0.9, 1.0, 0.0]]])) and not got.wide.any()


def _polygon(n, shift=0.0):
    ang = 2.0 * numpy.pi * (numpy.arange(n) + shift) / n
    return numpy.column_stack([numpy.ones(n), numpy.cos(ang), numpy.sin(ang)])


def test_a_reduced_cell_above_256_rows_is_the_rows_status():
    """a regular 200-gon under the identity against the 200-gon turned by half a side: the cell is a 400-gon, every row of it essential
    (a corner it cuts off is 1 / cos(pi / 200) - 1 / cos(pi / 400)... about 9e-5 deep, far above tol): 400 > 256 rows, the iteration stops
    with status ROWS and returns step 0"""
    got = _run([_polygon(200)], numpy.eye(2)[None], numpy.zeros((1, 2)), [[0]], [(0, _polygon(200, 0.5))])
    assert got.status == 'ROWS' and not got.converged and got.steps == 0 and len(got) == 1 and got.stats['cells'] == 1 and got.stats['items'] == 1
    assert got.rows_of(0).tobytes() == _polygon(200, 0.5).tobytes()


def test_limits_of_steps_and_cells():
    polys, Phi, phi, succ = xc.one_d_loop(4)
    pred, cells0 = ic.predecessors_of(succ), ic.one_d_cells0()
    full = _run(polys, Phi, phi, pred, cells0)
    for max_steps in (0, 1, 3):
        got = _run(polys, Phi, phi, pred, cells0, max_steps=max_steps)
        assert got.status == 'MAX_STEPS' and not got.converged and got.steps == max_steps and len(got) == 4 * (max_steps + 1)
        assert got.cell_rows.tobytes() == full.cell_rows[:full.cell_off[len(got)]].tobytes()
    got = _run(polys, Phi, phi, pred, cells0, max_cells=10)             # step 2 would make 12
    assert got.status == 'MAX_CELLS' and got.steps == 1 and len(got) == 8 and not got.converged
    got = _run(polys, Phi, phi, pred, cells0, max_rows_total=20)        # 2 rows per cell
    assert got.status == 'MAX_ROWS_TOTAL' and got.steps == 1 and len(got) == 8
    none = _run(polys, Phi, phi, pred, [])
    assert len(none) == 0 and none.converged and none.steps == 0 and none.status == 'CONVERGED'
    with pytest.raises(ValueError, match='step 0'):
        _run(polys, Phi, phi, pred, cells0, max_cells=3)
    # a chain that ends exactly at max_steps has converged: the items are listed before max_steps is tested.  R0 + (2, 0) lies inside R1, the
    # only cell of step 0, so step 1 is R0 whole (1 radius run + 8 rows = 9 LPs), and nothing precedes R0
    R0, R1 = xc.box_rows([0.0, 0.0], [1.0, 1.0]), xc.box_rows([1.5, -0.5], [3.5, 1.5])
    chain = ([R0, R1], numpy.tile(numpy.eye(2), (2, 1, 1)), numpy.array([[2.0, 0.0], [10.0, 0.0]]), [[], [0]], [(1, R1)])
    got = _run(*chain, max_steps=1)
    assert got.status == 'CONVERGED' and got.converged and got.steps == 1 and got.source.tolist() == [1, 0]
    assert got.rows_of(1).tobytes() == R0.tobytes() and got.stats['lps'] == 9
    got = _run(*chain, max_steps=0)
    assert got.status == 'MAX_STEPS' and not got.converged and len(got) == 1


def test_two_runs_give_identical_bits():
    polys, Phi, phi, pred, cells0, _, got, _ = _set(ic.SETS[1])
    again = _run(polys, Phi, phi, pred, cells0, max_steps=ic.MAX_STEPS)
    for name in ('cell_off', 'cell_rows', 'source', 'step', 'parent', 'wide', 'point'):
        assert getattr(again, name).tobytes() == getattr(got, name).tobytes(), name
    keys = ('items', 'cells', 'empty', 'lps', 'pivots', 'wide', 'cells_per_step')
    assert {k: again.stats[k] for k in keys} == {k: got.stats[k] for k in keys} and again.steps == got.steps


def test_graph_and_exits_passed_in_or_built_inside():
    sol, plant, graph, es, got, _ = _plant('c2')
    before = [(r.E.copy(), r.f.copy()) for r in sol.critical_regions]
    built = sol.invariant_set(plant['A'], plant['B'], plant['inputs'], max_steps=_MAX_STEPS['c2'], reduce_rows=False)
    for name in ('cell_off', 'cell_rows', 'source', 'step', 'parent', 'wide'):
        assert getattr(built, name).tobytes() == getattr(got, name).tobytes(), name
    assert all(numpy.array_equal(r.E, E) and numpy.array_equal(r.f, f) for r, (E, f) in zip(sol.critical_regions, before))
    with pytest.raises(ValueError, match='max_steps'):
        sol.invariant_set(plant['A'], plant['B'], plant['inputs'], max_steps=-1)


def test_merged_and_reduced_sources():
    sol, plant, _, _, _, _ = _plant('c3_l4')
    merged = sol.merge_regions(outputs=[0, 1])
    got = merged.invariant_set(plant['A'], plant['B'], [0, 1], max_steps=2)
    assert got.n_regions == len(merged) < len(sol) and len(got) > 0 and numpy.all(got.step[got.parent[got.parent >= 0]] == got.step[got.parent >= 0] - 1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        lp = solve_mpqp(pg.generate_mplp(4, 2, 10, seed=0), mpqp_algorithm.combinatorial)
    A, B = numpy.eye(2), numpy.zeros((2, 1))
    with pytest.raises(ValueError, match='remove_overlaps'):
        lp.invariant_set(A, B, [0])
    red = lp.remove_overlaps()
    stay = red.invariant_set(A, B, [0])                                  # theta+ = theta: nothing leaves
    assert len(stay) == 0 and stay.converged and stay.steps == 0
    out = red.invariant_set(A, B, [0], c=numpy.array([1000.0, 0.0]))     # every region leaves whole at once: no region has a predecessor
    assert len(out) == len(red) and out.converged and out.steps == 0 and out.stats['items'] == 0


def test_library_refusals():
    """MPC_ERR_INVALID (MpcError with the library's message) before any launch"""
    sq = xc.box_rows(numpy.zeros(2), numpy.ones(2))
    off, ef = xc.csr([sq, sq + numpy.array([0.5, 0, 0])])
    Phi, phi, xs = numpy.tile(0.5 * numpy.eye(2), (2, 1, 1)), numpy.zeros((2, 2)), numpy.array([[0.5, 0.5], [1.0, 0.5]])
    base = dict(off=off, ef=ef, Phi=Phi, phi=phi, xs=xs, poff=[0, 1, 2], pidx=[1, 0], coff=[0, 4], crow=sq, csrc=[0], tol=TOL, max_steps=2, max_cells=8,
                max_rows=64)
    call = lambda **kw: (lambda a: _lib.backward_exits(a['off'], a['ef'], a['Phi'], a['phi'], a['xs'], a['poff'], a['pidx'], a['coff'], a['crow'], a['csrc'],
                                                       a['tol'], a['max_steps'], a['max_cells'], a['max_rows']))(dict(base, **kw))
    r = call()
    assert r['status'] in range(5) and len(r['source']) >= 1 and r['step'][0] == 0
    assert call(coff=[0], crow=numpy.zeros((0, 3)), csrc=[])['converged']
    nan = ef.copy()
    nan[1, 1] = numpy.nan
    for kw, text in (({'tol': -1.0}, 'tol'), ({'tol': numpy.nan}, 'tol'), ({'ef': nan}, 'finite'), ({'crow': sq * 2.0}, 'unit'),
                     ({'Phi': numpy.full_like(Phi, numpy.inf)}, 'Phi must be finite'), ({'phi': phi + numpy.nan}, 'must be finite'), ({'xs': numpy.full_like(xs, numpy.nan)}, 'must be finite'),
                     ({'pidx': [1, 2]}, 'out of range'), ({'pidx': [-1, 0]}, 'out of range'), ({'csrc': [2]}, 'out of range'), ({'max_steps': -1}, 'max_steps'),
                     ({'off': [0, 0, 8]}, '1..256 rows'), ({'coff': [0, 0, 4], 'csrc': [0, 0]}, '1..256 rows'), ({'poff': [0, 2, 1], 'pidx': [0]}, 'pred_off'),
                     ({'max_cells': 0}, 'step 0')):
        with pytest.raises(_lib.MpcError, match=text):
            call(**kw)
