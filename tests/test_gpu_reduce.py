"""Removing redundant rows on the device: the hand cases of tests/reduce_cases.py; seeded sets against the independent CPU
reference at tol = 1e-6, up to n_theta = 16 and 512 rows; without the reference: membership of sampled points, vertices, volumes,
idempotence, determinism, start points, an unbounded polytope; and the consumers: the region difference past 256 rows, exit sets of the
solved programs c2 and c3, remove_overlaps, Solution.reduce_rows of a merged solution, the library's refusals."""
import time

import numpy
import pytest

import exit_cases as ec
import exit_reference as eref
import reduce_cases as rc
import reduce_reference as rr
import transition_reference as tref
from ppopt_amd import Solution, _lib, exit_sets as ex
from ppopt_amd.geometry import Polytope, reduce_polytopes, reduce_rows_of
from ppopt_amd.geometry.polytope_operations import hit_and_run_batch
from ppopt_amd.geometry.vertices import vertices_of_rows
from ppopt_amd.geometry.volume import volumes_of_rows

pytestmark = pytest.mark.gpu

TOL = rc.TOL
KNIFE_SHARE = 0.02       # of a case's polytopes
BAND = 1e-6              # points this close to a row are left out
BAND_SHARE = 0.01


# ---- 1. the hand cases -----------------------------------------------------------------------------------------------------------------
def test_hand_cases():
    for n_t in (2, 1):
        cases = [c for c in rc.hand_cases() if c[1].shape[1] == n_t + 1]
        off, ef = ec.csr([c[1] for c in cases])
        r = reduce_rows_of(off, ef, n_t, tol=TOL)
        want = numpy.concatenate([numpy.asarray(c[2], dtype=bool) for c in cases])
        assert r.kept.tolist() == want.tolist(), [c[0] for c in cases]
        assert r.rows.tobytes() == ef[want].tobytes()                      # the kept rows, bit for bit
        assert r.status.tolist() == [_lib.REDUCE_THIN if c[3] else _lib.REDUCE_OK for c in cases]
        assert r.stats['lps'] == sum(1 + (0 if c[3] else len(c[1])) for c in cases) and r.stats['thin'] == sum(c[3] for c in cases)
        for q, c in enumerate(cases):
            assert r.wide[q] <= (1 if c[0] == 'interval' else 0), c[0]
    sq = ec.box_rows([0, 0], [1, 1])
    p = Polytope(numpy.vstack([sq[:, 1:] * 3.0, [[2.0, 2.0]]]), numpy.vstack([sq[:, :1] * 3.0, [[4.0]]])).reduced(tol=TOL)      # x + y <= 2 touches
    assert p.A.tobytes() == (sq[:, 1:] * 3.0).tobytes() and p.b.tobytes() == (sq[:, :1] * 3.0).tobytes()


# ---- 2. seeded sets against the reference ------------------------------------------------------------------------------------------------
_CACHE = {}
_SINGLES = {'rows300': rc.rows_300, 'rows512': rc.rows_512}


def _set(case):
    """the polytopes, the reference's answer and the device run: computed once, shared, never modified"""
    if case not in _CACHE:
        polys = [_SINGLES[case]()] if case in _SINGLES else rc.seeded_set(*case)
        t0 = time.perf_counter()
        want = rr.reduce_reference(polys, TOL)
        ref_s = time.perf_counter() - t0
        off, ef = ec.csr(polys)
        got = reduce_rows_of(off, ef, ef.shape[1] - 1, tol=TOL)
        _CACHE[case] = (polys, want, got, off, ef, ref_s)
    return _CACHE[case]


def _against_the_reference(case):
    polys, want, got, off, ef, ref_s = _set(case)
    knife = [q for q, w in enumerate(want) if w.knife]
    s = got.stats
    print(f'{case}: {len(polys)} polytopes, {len(ef)} rows -> {s["rows_after"]}, {len(knife)} knife polytopes, reference {ref_s:.2f} s; device: {s["lps"]} LPs, '
          f'{s["pivots"] / max(1, s["lps"]):.2f} pivots per LP, {s["device_ms"]:.3f} ms ({1e6 * s["device_ms"] / max(1, s["lps"]):.0f} ns per LP), wall {s["wall_ms"]:.1f} ms')
    assert len(knife) <= KNIFE_SHARE * len(polys)
    for q, w in enumerate(want):
        assert int(got.status[q]) == (_lib.REDUCE_THIN if w.thin else _lib.REDUCE_OK), q
        assert int(got.wide[q]) == 0, q
        if q not in knife:
            mine = got.kept[off[q]:off[q + 1]]
            assert mine.tolist() == w.kept.tolist(), (q, numpy.flatnonzero(mine != w.kept).tolist(), w.row_radius[mine != w.kept].tolist())
    assert s['wide'] == 0 and s['thin'] == 0 and s['polytopes'] == len(polys) and s['lps'] == len(polys) + len(ef)
    assert got.rows.tobytes() == ef[got.kept].tobytes()
    return polys, want, got


@pytest.mark.parametrize('case', rc.SETS, ids=rc.IDS)
def test_seeded_sets_against_the_reference(case):
    """knife polytopes and unbounded runs with these seeds (the reference alone, run on the CPU): none"""
    polys, want, got = _against_the_reference(case)
    assert sum(int((~w.kept).sum()) for w in want) >= 2 * len(polys)


def test_300_rows_use_the_upper_mask_words():
    polys, want, got = _against_the_reference('rows300')
    assert len(polys[0]) == 300 and got.kept[256:].any() and not got.kept[256:].all() and got.kept[:64].any()


def test_512_rows_in_16_dimensions():
    """78,840 bytes of LDS, above the 48 KB a kernel gets without the attribute; the 384 tangent rows stay, the 128 outside go"""
    polys, want, got = _against_the_reference('rows512')
    assert polys[0].shape == (512, 17) and _lib.REDUCE_MAX_ROWS == 512
    assert int(got.kept.sum()) == int(want[0].kept.sum()) == 384


# ---- 3. without the reference -------------------------------------------------------------------------------------------------------------
_HALF = {1: 1.2, 2: 1.2, 3: 1.2, 5: 1.0, 16: 0.45}       # half-width of the sampling box around the Chebyshev centre


@pytest.mark.parametrize('case', rc.SETS, ids=rc.IDS)
def test_membership_of_sampled_points(case):
    polys, want, got, off, ef, _ = _set(case)
    n = case[0]
    rng = numpy.random.default_rng(200 + n)
    per = -(-20000 // len(polys))
    left = wrong = inside = total = 0
    for q, rows in enumerate(polys):
        _, _, centre = tref.chebyshev(rows)
        th = centre + rng.uniform(-_HALF[n], _HALF[n], (per, n))
        red = got.rows_of(q)
        m_orig, m_red = numpy.max(th @ rows[:, 1:].T - rows[:, 0], axis=1), numpy.max(th @ red[:, 1:].T - red[:, 0], axis=1)
        keep = numpy.min(numpy.abs(th @ rows[:, 1:].T - rows[:, 0]), axis=1) > BAND
        left += int((~keep).sum())
        wrong += int(numpy.sum(keep & ((m_orig <= 0.0) != (m_red <= 0.0))))
        inside += int(numpy.sum(keep & (m_orig <= 0.0)))
        total += per
    print(f'n_t = {n}: {total} points, {left} left out, {inside} inside, {wrong} disagree')
    assert total >= 20000 and left <= BAND_SHARE * total
    assert wrong == 0
    assert inside > 100 and total - left - inside > 100


@pytest.mark.parametrize('case', rc.SETS[:4], ids=rc.IDS[:4])
def test_vertices_and_volumes_agree(case):
    polys, want, got, off, ef, _ = _set(case)
    n = case[0]
    va, vb = vertices_of_rows(off, ef, n), vertices_of_rows(got.row_off, got.rows, n)
    assert numpy.all(va.status == 0) and numpy.all(vb.status == 0)
    for q in range(len(polys)):
        a, b = va.of(q), vb.of(q)
        assert len(a) >= n + 1 and len(b) >= n + 1
        d = numpy.linalg.norm(a[:, None, :] - b[None, :, :], axis=2)
        assert numpy.all(d.min(axis=1) <= 1e-9 * (1.0 + numpy.linalg.norm(a, axis=1))), q
        assert numpy.all(d.min(axis=0) <= 1e-9 * (1.0 + numpy.linalg.norm(b, axis=1))), q
    wa, wb = volumes_of_rows(off, ef, n, vertices=va), volumes_of_rows(got.row_off, got.rows, n, vertices=vb)
    assert numpy.all(wa.status == _lib.VOL_OK) and numpy.all(wb.status == _lib.VOL_OK)
    print(f'n_t = {n}: worst volume difference {float(numpy.max(numpy.abs(wa.volume - wb.volume) / (1.0 + wa.volume))):.3e}')
    assert numpy.all(numpy.abs(wa.volume - wb.volume) <= 1e-9 * (1.0 + wa.volume))


@pytest.mark.parametrize('case', [rc.SETS[1], rc.SETS[3], 'rows300'], ids=['n2', 'n5', 'rows300'])
def test_idempotent_deterministic_and_independent_of_the_start(case):
    polys, want, got, off, ef, _ = _set(case)
    n = ef.shape[1] - 1
    assert numpy.all(numpy.diff(got.row_off) <= numpy.diff(off)) and numpy.all(numpy.diff(got.row_off) >= n + 1)
    twice = reduce_rows_of(got.row_off, got.rows, n, tol=TOL)
    assert twice.kept.all() and twice.rows.tobytes() == got.rows.tobytes() and twice.row_off.tobytes() == got.row_off.tobytes()
    again = reduce_rows_of(off, ef, n, tol=TOL)
    for name in ('row_off', 'rows', 'kept', 'status', 'wide', 'point'):
        assert getattr(again, name).tobytes() == getattr(got, name).tobytes(), name
    assert {k: again.stats[k] for k in ('lps', 'pivots', 'wide', 'thin')} == {k: got.stats[k] for k in ('lps', 'pivots', 'wide', 'thin')}
    # the saved point is interior, and a run that starts there, or at the Chebyshev centre, gives the same masks
    for q, rows in enumerate(polys):
        assert numpy.all(rows[:, 1:] @ got.point[q] < rows[:, 0])
    for start in (got.point, numpy.array([tref.chebyshev(rows)[2] for rows in polys])):
        other = reduce_rows_of(off, ef, n, tol=TOL, start=start)
        assert other.kept.tobytes() == got.kept.tobytes() and other.status.tobytes() == got.status.tobytes()


def test_an_unbounded_polytope_keeps_its_rows():
    """a strip and a cone at n_theta = 2: no row may go; a run is unbounded (wide) or ends by the stop rule, kept either way"""
    strip = numpy.array([[1.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    cone = numpy.array([[1.0, 1.0, 0.0], [1.0, 0.0, 1.0]])
    half = numpy.array([[1.0, 1.0, 0.0], [2.0, 1.0, 0.0]])               # one half-plane twice over: x <= 2 goes, x <= 1 stays
    off, ef = ec.csr([strip, cone, half])
    r = reduce_rows_of(off, ef, 2, tol=TOL)
    assert r.kept.tolist() == [True, True, True, True, True, False] and r.status.tolist() == [0, 0, 0]
    assert r.stats['wide'] == int(r.wide.sum()) and numpy.all(r.wide >= 0)
    got = reduce_polytopes([Polytope(strip[:, 1:], strip[:, :1])], tol=TOL)
    assert got.kept.all()


# ---- 4. the consumers ---------------------------------------------------------------------------------------------------------------------
def test_the_row_limit_falls_with_reduce_rows():
    """the source of 200 rows and the cutter of 100 of tests/reduce_cases.py: the children reach 300 rows"""
    from test_reduce_cpu import same_sets
    polys, Phi, phi, succ = rc.many_rows_difference()
    off, ef = ec.csr(polys)
    with pytest.raises(ValueError, match='exit_sets: a piece has more than 256 rows after round 1'):
        ex.exit_pieces(off, ef, Phi, phi, 2, succ, tol=TOL)
    with pytest.raises(ValueError, match='exit_sets: a piece has more than 256 rows after round 1'):
        ex.exit_pieces(off, ef, Phi, phi, 2, succ, tol=TOL, reduce_rows=False)
    got = ex.exit_pieces(off, ef, Phi, phi, 2, succ, tol=TOL, reduce_rows=True)
    want, knife = eref.exit_reference(polys, Phi, phi, succ, TOL)          # the difference without a row limit
    s = got.stats
    print(f'{len(got)} pieces, {sum(len(p[1]) for p in want)} rows without reduction, {int(got.piece_off[-1])} with; {s["reduce_lps"]} reduction LPs in '
          f'{s["reduce_ms"]:.3f} ms ({1e6 * s["reduce_ms"] / s["reduce_lps"]:.0f} ns per LP), {s["rows_removed"]} rows removed')
    assert not knife and len(want) == 101 and max(len(p[1]) for p in want) == 300
    assert got.source.tolist() == [p[0] for p in want] and got.whole.tolist() == [False, True]
    assert int(numpy.diff(got.piece_off).max()) <= 256 and s['rows_removed'] > 100 * 100 and s['reduce_lps'] > 100 * 200
    n_mine, n_theirs = same_sets([got.rows_of(k) for k in range(len(got))], [p[1] for p in want])
    assert n_mine == n_theirs == 101


def _near_a_boundary(e, th):
    """[n] bool: the point lies within BAND of some row of some piece"""
    out = numpy.zeros(len(th), dtype=bool)
    chunk = max(1, (1 << 24) // max(1, len(e.piece_rows)))
    for a in range(0, len(th), chunk):
        out[a:a + chunk] = numpy.min(numpy.abs(e.piece_rows[:, 1:] @ th[a:a + chunk].T - e.piece_rows[:, :1]), axis=0) <= BAND
    return out


def _solved(name):
    import test_gpu_exit_sets as tge
    return tge._case(name), tge


@pytest.mark.parametrize('name', ['c2', 'c3_l4'])
def test_exit_sets_of_the_plants(name):
    (sol, plant, graph, plain), tge = _solved(name)
    t0 = time.perf_counter()
    during = sol.exit_sets(plant['A'], plant['B'], plant['inputs'], graph=graph, reduce_rows=True)
    after = plain.reduced()
    print(f'{name}: {len(plain)} pieces of {int(plain.piece_off[-1])} rows; reduced during the rounds: {len(during)} pieces of {int(during.piece_off[-1])} rows, '
          f'{during.stats["reduce_lps"]} LPs in {during.stats["reduce_ms"]:.3f} ms; reduced afterwards: {int(after.piece_off[-1])} rows, {after.stats["reduce_lps"]} LPs in '
          f'{after.stats["reduce_ms"]:.3f} ms; {time.perf_counter() - t0:.1f} s')
    assert int(during.piece_off[-1]) <= int(plain.piece_off[-1]) and int(after.piece_off[-1]) <= int(plain.piece_off[-1])
    assert len(after) == len(plain) and after.source.tobytes() == plain.source.tobytes() and after.whole.tobytes() == plain.whole.tobytes()
    assert numpy.all(numpy.diff(after.piece_off) <= numpy.diff(plain.piece_off)) and numpy.all(after.wide >= plain.wide)
    assert after.region_off is plain.region_off and after.region_rows is plain.region_rows
    assert during.n_regions == plain.n_regions and numpy.all(numpy.diff(during.source) >= 0)
    # states that leave in one simulated step
    R = len(sol)
    chains = -(-5000 // R)
    pts = hit_and_run_batch([Polytope(r.E, r.f) for r in sol.critical_regions], chains=chains, samples=1, n_steps=50, seed=tge.SIM_SEED)[:, :, 0, :]
    th0 = numpy.ascontiguousarray(pts.transpose(1, 0, 2).reshape(-1, pts.shape[-1])[:5000])
    exact = Solution(sol.program, sol.critical_regions, is_overlapping=False, point_location_tolerance=0.0)
    exact.is_complete = sol.is_complete
    region = exact.simulate(th0, 2, plant['A'], plant['B'], plant['inputs'], locate='scan').region
    th = th0[(region[:, 0] >= 0) & (region[:, 1] < 0)]
    near = numpy.zeros(len(th), dtype=bool)
    for e in (plain, during, after):
        if len(e) and len(th):
            near |= _near_a_boundary(e, th)
    hit = plain.contains(th) >= 0
    print(f'{name}: {len(th0)} points, {len(th)} leave in one step, {int(near.sum())} left out, {int(hit[~near].sum())} found by the plain pieces')
    assert int(near.sum()) <= BAND_SHARE * len(th0)
    for e in (during, after):
        numpy.testing.assert_array_equal((e.contains(th) >= 0)[~near], hit[~near])
    # volumes, wherever both give an answer
    v0, v1, v2 = plain.volumes(), during.volumes(), after.volumes()
    for v in (v1, v2):
        both = ~numpy.isnan(v0.exit) & ~numpy.isnan(v.exit)
        assert both.any()
        assert numpy.all(numpy.abs(v.exit[both] - v0.exit[both]) <= 1e-9 * (1.0 + v0.exit[both]))
    print(f'{name}: pieces without a volume: {int(numpy.isnan(v0.piece).sum())} plain, {int(numpy.isnan(v1.piece).sum())} reduced during, '
          f'{int(numpy.isnan(v2.piece).sum())} reduced afterwards')


def test_remove_overlaps_with_reduce_rows():
    import test_gpu_overlap as tgo
    prog, sol, plain = tgo._solved('mplp')
    red = sol.remove_overlaps(reduce_rows=True)
    rows = lambda s: sum(len(r.E) for r in s.critical_regions)
    st = red.overlap_info['stats']
    print(f'{len(sol)} regions -> {len(plain)} pieces of {rows(plain)} rows, {len(red)} of {rows(red)} rows with reduce_rows ({st["reduce_lps"]} LPs, '
          f'{st["rows_removed"]} rows removed)')
    assert rows(red) <= rows(plain) and st['reduce_lps'] > 0 and 'reduce_lps' not in plain.overlap_info['stats']
    assert not red.is_overlapping and red.overlap_info['source'] is sol
    ca, cb = plain.coverage_volume(), red.coverage_volume()
    assert ca.ok and cb.ok and abs(ca.total - cb.total) <= 1e-9 * (1.0 + ca.total)
    th, _ = tgo._theta_points(prog, plain, 5000, 6)
    src_a = numpy.array([-1] + [r.source for r in plain.critical_regions])[plain.get_region_batch(th) + 1]
    src_b = numpy.array([-1] + [r.source for r in red.critical_regions])[red.get_region_batch(th) + 1]
    numpy.testing.assert_array_equal(src_a, src_b)
    if len(red) == len(plain):
        numpy.testing.assert_array_equal(plain.get_region_batch(th), red.get_region_batch(th))
    x_a, _ = plain.evaluate_batch(th)
    x_b, _ = red.evaluate_batch(th)
    numpy.testing.assert_array_equal(x_a, x_b)
    # the finished solution, reduced in one call: the same answers again
    late = plain.reduce_rows()
    assert rows(late) <= rows(plain) and len(late) == len(plain) and late.overlap_info is plain.overlap_info
    numpy.testing.assert_array_equal(late.get_region_batch(th), plain.get_region_batch(th))


def test_a_merged_solution_reduced_locates_and_evaluates_like_its_source():
    (sol, plant, _, _), tge = _solved('c3_l4')
    merged = sol.merge_regions(outputs=[0, 1])
    red = merged.reduce_rows()
    rows = lambda s: sum(len(r.E) for r in s.critical_regions)
    info = red.reduce_info
    print(f'{len(merged)} merged regions of {rows(merged)} rows -> {rows(red)} rows; {info["stats"]["lps"]} LPs in {info["stats"]["device_ms"]:.3f} ms, '
          f'{int((info["status"] == _lib.REDUCE_THIN).sum())} thin, {int((info["wide"] > 0).sum())} wide')
    assert len(red) == len(merged) and rows(red) <= rows(merged) and red.merge_info is merged.merge_info
    assert [r.members for r in red.critical_regions] == [r.members for r in merged.critical_regions]
    for a, b in zip(red.critical_regions[:20], merged.critical_regions[:20]):
        numpy.testing.assert_array_equal(a.A, b.A)
        numpy.testing.assert_array_equal(a.b, b.b)
    pts = hit_and_run_batch([Polytope(r.E, r.f) for r in merged.critical_regions], chains=-(-5000 // len(merged)), samples=1, n_steps=50, seed=11)[:, :, 0, :]
    th = numpy.ascontiguousarray(pts.reshape(-1, pts.shape[-1])[:5000])
    rows_m = numpy.vstack([numpy.hstack([numpy.asarray(r.f, dtype=float).reshape(-1, 1), numpy.asarray(r.E, dtype=float)]) for r in merged.critical_regions])
    away = numpy.min(numpy.abs(th @ rows_m[:, 1:].T - rows_m[:, 0]) / numpy.linalg.norm(rows_m[:, 1:], axis=1), axis=1) > 1e-4
    assert away.sum() > 1000          # (a point counts as near when any row of any of the regions passes within 1e-4)
    x_a, reg_a = merged.evaluate_batch(th[away])
    x_b, reg_b = red.evaluate_batch(th[away])
    numpy.testing.assert_array_equal(reg_a, reg_b)
    numpy.testing.assert_array_equal(x_a, x_b)
    assert (reg_a >= 0).all()


def test_library_refusals():
    """MPC_ERR_INVALID (MpcError with the library's message) before any launch; an empty batch is fine"""
    sq = ec.box_rows(numpy.zeros(2), numpy.ones(2))
    off, ef = ec.csr([sq, sq])
    call = lambda **kw: _lib.reduce_rows(kw.get('off', off), kw.get('ef', ef), kw.get('start', None), kw.get('tol', TOL))
    kept, status, wide, point, stats = call()
    assert kept.all() and status.tolist() == [0, 0] and stats['polytopes'] == 2 and stats['lps'] == 10 and stats['thin'] == 0
    kept, status, wide, point, stats = call(off=[0], ef=numpy.zeros((0, 3)))
    assert len(kept) == 0 and len(status) == 0 and stats['polytopes'] == 0 and stats['ms'] == 0.0
    nan = ef.copy()
    nan[1, 1] = numpy.nan
    big = numpy.tile(sq, (129, 1))
    for kw, text in (({'tol': -1.0}, 'tol must be finite'), ({'tol': numpy.nan}, 'tol must be finite'), ({'ef': nan}, 'finite with unit normals'),
                     ({'ef': ef * 2.0}, 'finite with unit normals'), ({'start': numpy.array([[numpy.inf, 0.0], [0.0, 0.0]])}, 'start must be finite'),
                     ({'off': [0, 0, 8]}, '1..512 rows'), ({'off': [0, 516], 'ef': big}, '1..512 rows'),
                     ({'off': [0, 2], 'ef': numpy.hstack([numpy.ones((2, 1)), numpy.eye(17)[:2]])}, 'n_t must lie in 1..16')):
        with pytest.raises(_lib.MpcError, match='mpc_reduce_rows.*' + text):
            call(**kw)
    with pytest.raises(_lib.MpcError, match='row_off'):
        call(off=[1, 4, 8])
