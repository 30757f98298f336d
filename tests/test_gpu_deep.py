"""The benchmarked solves themselves against the REAL reference, candidate by candidate (tests/golden/c4_deep.npz, c3_deep.npz:
every candidate of every benchmarked level run through the reference's own check_feasibility / check_optimality /
gen_cr_from_active_set by oracle/ref_harness/gen_deep_goldens.py), and config 5 against its golden verdicts.

Bars (north_star): candidate lists, verdicts, the set of region active sets and every region's omega / lambda / regular index
sets bit-exact; coefficients within 1e-8.  A difference is accepted only for an active set listed in conftest.KNIFE_EDGE_* and
knife-edge by conftest.is_knife_edge; the number used is recorded.
"""
import os
import warnings

import numpy
import pytest

from conftest import GOLDEN, consume_exception, is_knife_edge, load_golden, rel_err, rows_match

pytestmark = pytest.mark.gpu

COEF_TOL = 1e-8


def unpad(row):
    return [int(v) for v in row if v >= 0]


def digest(arrs):
    return numpy.array([[a.sum(), (a * a).sum()] for a in arrs])


def run_deep(name, base_golden, oracle):
    from ppopt_amd.region_batch import RegionBatch
    from test_gpu_parity import engine_from_golden
    path = os.path.join(GOLDEN, name + '_deep.npz')
    if not os.path.exists(path):
        pytest.skip(f'{name}_deep.npz has not been generated')
    d = numpy.load(path)
    g = load_golden(base_golden)
    P = oracle.problem_from_golden(g)
    n_levels = sum(1 for key in d.files if key.endswith('_verdict') and key.startswith('L'))
    eng = engine_from_golden(g)
    eng.pruned_clear()
    eng.frontier_root()
    offenders = []
    used = 0
    regions = {}
    n_cand = 0
    for lev in range(n_levels):
        gen = lev + 1 != n_levels
        st = eng.level_run(gen)
        cands, status = eng.frontier_get(), eng.level_status()
        gc, gv = d[f'L{lev}_cands'].astype(numpy.int32), d[f'L{lev}_verdict']
        if numpy.array_equal(cands, gc):
            differing = [(tuple(int(v) for v in cands[j]), int(status[j]), int(gv[j]), float(d[f'L{lev}_cond'][j])) for j in numpy.flatnonzero(status != gv).tolist()]
        else:
            # only a changed verdict upstream can change the list: it must then be a listed exception, and every candidate both sides
            # visit is still compared (no level is skipped once an exception has been consumed)
            assert used > 0 or offenders, f'{name} level {lev + 1}: candidate list differs from the reference run'
            ref_v = {tuple(r): (int(v), float(c)) for r, v, c in zip(gc.tolist(), gv.tolist(), d[f'L{lev}_cond'].tolist())}
            differing = [(tuple(c), int(v), ref_v[tuple(c)][0], ref_v[tuple(c)][1]) for c, v in zip(cands.tolist(), status.tolist())
                         if tuple(c) in ref_v and ref_v[tuple(c)][0] != int(v)]
        for key, v_gpu, v_ref, cond in differing:
            if consume_exception('verdict', name + '_deep', key, f'gpu {v_gpu} reference {v_ref}') and is_knife_edge(P, list(key)):
                used += 1
            else:
                offenders.append(('verdict', lev + 1, key, v_gpu, v_ref, cond))
        n_cand += len(cands)
        if st.n_regions:
            hd, hi, er, kk, slots = eng.level_regions_slots()
            for r in RegionBatch(hd, hi, er, eng.n_x, eng.n_t, eng.n_c, eng.n_tc, kk, slots).regions():
                regions[tuple(r.active_set)] = r
        if not gen or st.n_children == 0:
            break
        eng.frontier_advance()
    eng.close()
    assert n_cand == sum(len(d[f'L{i}_verdict']) for i in range(n_levels))
    # ---- the region set: exactly the reference's active sets -----------------------------------------------------------
    ref_keys = [tuple(int(v) for v in row[:k]) for row, k in zip(d['R_active'], d['R_k'])]
    ref_index = {key: i for i, key in enumerate(ref_keys) if len(key) > 0}
    for key in set(ref_index) ^ set(regions):
        side = 'reference only' if key in ref_index else 'gpu only'
        if not (consume_exception('region', name + '_deep', key, side) and is_knife_edge(P, list(key))):
            offenders.append(('region', key, side))
    # ---- every region: index sets bit-exact, coefficient digests within 1e-8 per element ---------------------------------
    S = d['S_digest']
    SW = d['S_wdigest'] if 'S_wdigest' in d.files else None      # order-sensitive: sum (m + 1) a_m (oracle/ref_harness/add_weighted_digest.py)
    assert SW is not None, f'{name}_deep.npz carries no order-sensitive digest'
    for key, r in regions.items():
        i = ref_index.get(key)
        if i is None:
            continue
        same = (r.omega_set == unpad(d['R_omega'][i]) and r.lambda_set == unpad(d['R_lambda'][i])
                and r.regular_set == [unpad(d['R_regular_idx'][i]), unpad(d['R_regular_con'][i])] and r.E.shape[0] == int(d['R_nE'][i]))
        if not same:
            if not (consume_exception('facets', name + '_deep', key) and is_knife_edge(P, list(key), cond_limit=1e6)):
                offenders.append(('facets', key))
            continue
        arrs = (r.A, r.b, r.C, r.d, r.E, r.f)
        got = digest(arrs)
        for j, a in enumerate(arrs):
            # every element within tol (1 + |ref|)  =>  |sum - sum_ref| <= tol (n + sum|ref|) <= tol (n + sqrt(n * sumsq_ref))
            bound = COEF_TOL * (a.size + numpy.sqrt(a.size * S[i, j, 1]))
            assert abs(got[j, 0] - S[i, j, 0]) <= bound, (name, key, 'sum', j)
            assert abs(got[j, 1] - S[i, j, 1]) <= 4 * COEF_TOL * (a.size + S[i, j, 1]), (name, key, 'sumsq', j)
            # position-weighted sum: swapped rows of A / C / E (which sum and sum of squares cannot see) change it.
            # every element within tol (1 + |ref|)  =>  |w . (a - ref)| <= tol (sum w + sqrt(sum w^2 * sumsq_ref)),  w = 1..n
            n_el = a.size
            w1, w2 = n_el * (n_el + 1) / 2.0, n_el * (n_el + 1) * (2 * n_el + 1) / 6.0
            wsum = float(numpy.dot(numpy.arange(1, n_el + 1, dtype=numpy.float64), numpy.asarray(a, dtype=numpy.float64).ravel()))
            assert abs(wsum - SW[i, j]) <= COEF_TOL * (w1 + numpy.sqrt(w2 * S[i, j, 1])), (name, key, 'weighted sum', j)
    # ---- the strided sample with full coefficient arrays ---------------------------------------------------------------------
    for pos, i in enumerate(d['F_index'].tolist()):
        key = ref_keys[i]
        r = regions.get(key)
        if r is None or key not in ref_index:
            continue
        k, ne = int(d['R_k'][i]), int(d['R_nE'][i])
        assert rel_err(r.A, d['F_A'][pos]) <= COEF_TOL and rel_err(r.b.ravel(), d['F_b'][pos]) <= COEF_TOL, key
        assert rel_err(r.C, d['F_C'][pos][:k]) <= COEF_TOL and rel_err(r.d.ravel(), d['F_d'][pos][:k]) <= COEF_TOL, key
        if r.E.shape[0] == ne:
            assert rows_match(r.E, r.f, d['F_E'][pos][:ne], d['F_f'][pos][:ne], COEF_TOL), key
    assert not offenders, f'{name}: {len(offenders)} differences from the reference run that are not listed knife-edge exceptions: {offenders[:40]}'
    return n_cand, len(regions)


def test_config4_every_candidate_and_region_equals_the_reference(oracle):
    """bench.py's workload: generate_mpqp(20,8,20,seed=0), levels 1-5 -- 1,151,349 candidates, every one with the reference's
    verdict, and exactly the reference's regions."""
    n_cand, n_reg = run_deep('c4', 'c4_rand_20_8_20_s0', oracle)
    assert n_cand == 1151349


def test_config3_every_candidate_and_region_equals_the_reference(oracle):
    """bench.py --workload c3: quad tank N=10, levels 1-4."""
    run_deep('c3', 'c3_quadtank_n10', oracle)


def test_config5_verdicts_equal_the_reference_where_the_kkt_matrix_is_well_conditioned(oracle):
    """Config 5 (control allocation, Q of rank 4 of 8): the reference decides its first level with KKT matrices of condition
    4e16 and aborts with LinAlgError, so its own trace (c5_control_allocation.npz) is 29 candidates long.  c5_deep.npz
    (oracle/ref_harness/gen_deep_goldens.py c5) holds the reference's verdict and cond(KKT) for every candidate of the tree
    walked with ill-conditioned sets expanded -- 5,102 candidates, 4,395 of them decided by the reference before any KKT solve
    or with cond < 1e10.  Every such candidate the device visits must carry the reference's verdict, and every such region
    the reference's index sets."""
    from test_gpu_parity import engine_from_golden, run_levels
    g = load_golden('c5_control_allocation')
    d = load_golden('c5_deep')
    P = oracle.problem_from_golden(g)
    eng = engine_from_golden(g)
    levels, regions = run_levels(eng)
    got = {}
    for cands, status, _ in levels:
        for cand, v in zip(cands.tolist(), status.tolist()):
            got[tuple(cand)] = int(v)
    checked = n_singular_for_not_optimal = 0
    offenders = []
    import json
    listed_4_for_1 = {tuple(a) for a in json.load(open(os.path.join(GOLDEN, 'c5_singular_for_not_optimal.json')))['active_sets']}
    assert len(listed_4_for_1) == 106
    for i in range(int(d['n_levels'])):
        for cand, v, cond in zip(d[f'L{i}_cands'].tolist(), d[f'L{i}_verdict'].tolist(), d[f'L{i}_cond'].tolist()):
            key = tuple(cand)
            if not (numpy.isnan(cond) or cond < 1e10) or key not in got:
                continue
            checked += 1
            # MPC_SINGULAR_KKT (4) is "feasible, KKT matrix singular: no region, children expanded" (include/mpcombi.h): the device
            # poses the KKT system before the optimality question and cannot answer it for a singular matrix; the reference asks
            # check_optimality first (an LP, no KKT solve) and says 1, "feasible, not optimal" -- the same outcome for the driver
            # (no region, not pruned, children expanded).
            # Accepted for the 106 active sets LISTED in tests/golden/c5_singular_for_not_optimal.json (tools/c5_singular_list.py) and nothing else.
            same = got[key] == int(v) or (got[key] == 4 and int(v) == 1 and key in listed_4_for_1)
            n_singular_for_not_optimal += int(got[key] == 4 and int(v) == 1)
            if not same:
                if not (consume_exception('verdict', 'c5_deep', key, f'gpu {got[key]} reference {v}') and is_knife_edge(P, cand)):
                    offenders.append(('verdict', key, got[key], int(v), cond))
    mine = {tuple(r.active_set): r for r in regions}
    n_regions = n_tight = 0
    from conftest import kkt_condition
    for i in range(len(d['R_k'])):
        key = tuple(int(v) for v in d['R_active'][i][:int(d['R_k'][i])])
        r = mine.get(key)
        if r is None:
            continue      # reported above as a verdict difference if the device visited it
        n_regions += 1
        same = (r.omega_set == unpad(d['R_omega'][i]) and r.lambda_set == unpad(d['R_lambda'][i])
                and r.regular_set == [unpad(d['R_regular_idx'][i]), unpad(d['R_regular_con'][i])] and r.E.shape[0] == int(d['R_nE'][i]))
        if not same:
            if not (consume_exception('facets', 'c5_deep', key) and is_knife_edge(P, list(key), cond_limit=1e6)):
                offenders.append(('facets', key))
            continue
        # cond < 1e10: the reference's own solve carries up to cond * eps of error: 1e-8 relative where cond(KKT) <= 2.5e7, 4e-16 * cond above
        # (at most 1e-6) -- round 5: per region, by its own condition number, instead of 1e-6 for all
        tol = min(1e-6, max(COEF_TOL, 4e-16 * kkt_condition(P, list(key))))
        n_tight += int(tol == COEF_TOL)
        for j, a in enumerate((r.A, r.b, r.C, r.d, r.E, r.f)):
            S = d['S_digest'][i, j]
            assert abs(a.sum() - S[0]) <= tol * (a.size + numpy.sqrt(a.size * S[1])), ('c5', key, j, tol)
            n_el = a.size      # the order-sensitive digest (sum (m + 1) a_m), same bound scheme
            wsum = float(numpy.dot(numpy.arange(1, n_el + 1, dtype=numpy.float64), numpy.asarray(a, dtype=numpy.float64).ravel()))
            assert abs(wsum - d['S_wdigest'][i, j]) <= tol * (n_el * (n_el + 1) / 2.0 + numpy.sqrt(n_el * (n_el + 1) * (2 * n_el + 1) / 6.0 * S[1])), ('c5', key, 'weighted', j, tol)
    eng.close()
    print(f'c5: {checked} pinned candidates visited, {n_singular_for_not_optimal} of them singular-for-not-optimal, {n_regions} regions compared, {n_tight} of them at 1e-8')
    assert not offenders, (len(offenders), numpy.unique([(o[2], o[3]) for o in offenders if o[0] == 'verdict'], axis=0, return_counts=True), offenders[:40])
    assert checked >= 2000 and n_regions >= 300, (checked, n_regions)


def test_out_of_spare_region_slots_repeats_the_solve_and_loses_nothing(monkeypatch):
    """late optimal candidates beyond the spare slots of an overlapped region launch used to be demoted to
    'feasible'.  Now the level fails with MPC_ERR_CAPACITY and the driver repeats the solve without the overlap.  Forced here:
    every level overlaps (MPC_ROVERLAP_MIN=0), five optimal candidates are held back for the late path (MPC_TEST_LATE=5) and the
    launch reserves 1,030 slots fewer than it would (MPC_TEST_SPARE)."""
    from ppopt_amd import Solver, _lib
    from ppopt_amd.mp_solvers import mpqp_hip_combinatorial
    from test_host_logic import build_program
    if os.environ.get('MPC_FORCE_V1') == '1':
        pytest.skip('the LDS-engine kernels (MPC_FORCE_V1=1) have no overlapped region stage')

    def solve():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            prog = build_program(load_golden('rand_6_3_12_s1'), Solver())
        sol = mpqp_hip_combinatorial.solve(prog)
        eng = prog.engine(0)
        return {tuple(r.active_set): r for r in sol.critical_regions}, prog, eng

    base, _, _ = solve()
    with monkeypatch.context() as m:
        m.setenv('MPC_TEST_LATE', '5')
        m.setenv('MPC_ROVERLAP_MIN', '0')
        m.setenv('MPC_TEST_SPARE', '1030')
        # the level itself reports the shortage ...
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            prog = build_program(load_golden('rand_6_3_12_s1'), Solver())
        with pytest.raises(_lib.MpcCapacityError):
            mpqp_hip_combinatorial._solve(prog)
        prog.release_engine()
        # ... and the public driver repeats and returns everything
        other, _, _ = solve()
    assert set(other) == set(base) and len(base) > 20
    for key, r1 in base.items():
        r2 = other[key]
        assert r1.omega_set == r2.omega_set and r1.lambda_set == r2.lambda_set and r1.regular_set == r2.regular_set
        for fld in ('A', 'b', 'C', 'd', 'E', 'f'):
            assert numpy.allclose(getattr(r1, fld), getattr(r2, fld), rtol=0, atol=COEF_TOL), (key, fld)


@pytest.mark.parametrize('name', ['transport_mpqp', 'c1_transport_mplp', 'rand_5_3_8_s3'])
def test_upop_payload_of_a_device_solution_describes_the_reference_solution(name):
    """SURVEY.md 8(f)4 on the device path: the program is presolved and solved on the GPU, exported in the reference's uPOP format
    (ppopt_amd.upop.upop_payload), and the export is compared with the fixture the reference produced for ITS solution of the
    same program (tests/golden/export_*.npz).  The two solutions list their regions in different orders, so the comparison is
    order-free: the same set of fundamental hyperplanes and of fundamental functions (to 1e-8, up to the sign the first
    occurrence fixes), the same number of rows, and every region's rows rebuilt from the tables equal to its E, f."""
    from ppopt_amd import MPLP_Program, MPQP_Program, problem_generator as pg
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    from ppopt_amd.upop import upop_payload as up
    g = numpy.load(os.path.join(GOLDEN, f'export_{name}.npz'))
    d = {'transport_mpqp': pg.transport_mpqp_data, 'c1_transport_mplp': pg.transport_mplp_data,
         'rand_5_3_8_s3': lambda: pg.generate_mpqp_data(5, 3, 8, 3)}[name]()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if d['Q'] is None:
            prog = MPLP_Program(d['A'], d['b'], d['c'], d['H'], d['A_t'], d['b_t'], d['F'], equality_indices=list(d['equality_indices']))
        else:
            prog = MPQP_Program(d['A'], d['b'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], d['F'], equality_indices=list(d['equality_indices']))
        sol = solve_mpqp(prog, mpqp_algorithm.combinatorial)
    t = up.upop_tables(sol)
    assert t['num_regions'] == len(g['R_k'])
    # (the NUMBER of rows of a region can differ by exact-duplicate rows: the reference drops rows that are bit-for-bit equal,
    #  constraint_utilities.py:125-134, which is an accident of the arithmetic; the row SETS are what is compared)

    def canon(rows, digits):
        out = set()
        for r in rows:
            nz = numpy.flatnonzero(numpy.abs(r) > 1e-9)
            s = 1.0 if len(nz) == 0 or r[nz[0]] > 0 else -1.0
            out.add(tuple(numpy.round(s * r, digits) + 0.0))
        return out
    mine = numpy.hstack([t['E'], t['f']])[t['fundamental_c']]
    ref = numpy.hstack([g['M_constraint_block'], g['M_constraint_vector']])[g['T_fundamental_c']]
    assert canon(mine, 7) == canon(ref, 7)
    mine_f = numpy.hstack([t['A'], t['b']])[t['fundamental_f']]
    ref_f = numpy.hstack([g['M_function_block'], g['M_function_vec']])[g['T_fundamental_f']]
    assert canon(mine_f, 6) == canon(ref_f, 6)
    # the tables reproduce every region's own rows
    planes = numpy.hstack([t['E'], t['f']])[t['fundamental_c']]
    for j, r in enumerate(sol.critical_regions):
        lo, hi = t['region_boundary_index'][j], t['region_boundary_index'][j + 1]
        rebuilt = numpy.array([t['parity_c'][i] * planes[t['original_c'][i]] for i in range(lo, hi)])
        assert numpy.allclose(rebuilt, numpy.hstack([r.E, r.f]), rtol=0, atol=2e-9)
    text = up.payload_cpp(sol, 'double')
    assert text.count('\n') == str(g['payload_cpp']).count('\n') and f'const int num_regions = {len(g["R_k"])};' in text
    assert f'const int num_fundamental_hyper_planes = {len(g["T_fundamental_c"])};' in text


# ---- the dense Hessian factor and the one-off Schur blocks on the matrix cores (csrc/setup_mfma.hip) ---------------------------
def _random_program(rng, nx, nt, nc, psd_rank=None):
    R = rng.standard_normal((nx if psd_rank is None else psd_rank, nx))
    Q = R.T @ R + (numpy.eye(nx) if psd_rank is None else 0.0)
    A = numpy.round(rng.standard_normal((nc, nx)) * 3) / 2
    A[rng.random((nc, nx)) < 0.3] = 0.0
    return dict(A=A, b=rng.random((nc, 1)) + 1.0, F=numpy.round(rng.standard_normal((nc, nt)) * 2) / 2, c=rng.standard_normal((nx, 1)),
                H=rng.standard_normal((nx, nt)), Q=Q, A_t=numpy.vstack([numpy.eye(nt), -numpy.eye(nt)]), b_t=numpy.ones((2 * nt, 1)))


@pytest.mark.parametrize('shape', [(20, 8, 47), (5, 3, 8), (16, 2, 16), (17, 4, 33), (40, 10, 100), (64, 6, 130), (33, 3, 49)])
def test_mfma_setup_blocks_equal_numpy(shape):
    """mpc_create forms W = A Q^-1 A', UV, Gt = A Q^-1, X0H = -Q^-1 [c | H] and A A' on the device with
    v_mfma_f64_16x16x4_f64 tiles (blocked Cholesky, two blocked triangular solves, tile products).  Compared with numpy on
    shapes with one to five 16-row blocks per dimension, including exact multiples of 16; tolerance 1e-11 x cond(Q) relative."""
    from ppopt_amd import _lib
    nx, nt, nc = shape
    d = _random_program(numpy.random.default_rng(nx * 1000 + nc), nx, nt, nc)
    eng = _lib.Engine(d['A'], d['b'], d['F'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], 0)
    Qi = numpy.linalg.inv(d['Q'])
    cond = numpy.linalg.cond(d['Q'])
    want = {0: d['A'] @ Qi @ d['A'].T, 1: numpy.hstack([d['A'] @ Qi @ d['c'] + d['b'], d['A'] @ Qi @ d['H'] + d['F']]),
            2: d['A'] @ Qi, 3: -Qi @ numpy.hstack([d['c'], d['H']]), 4: d['A'] @ d['A'].T}
    for which, ref in want.items():
        got = eng.program_block(which)
        assert got.shape == ref.shape, (which, got.shape)
        err = numpy.max(numpy.abs(got - ref)) / (1.0 + numpy.max(numpy.abs(ref)))
        assert err <= 1e-11 * max(cond, 1.0), (shape, which, err, cond)
    W = eng.program_block(0)
    assert numpy.array_equal(W, W.T)      # symmetric by construction (Y'Y)
    eng.close()


@pytest.mark.parametrize('shape', [(20, 4, 40, 1), (15, 2, 32, 10), (24, 3, 49, 16), (30, 8, 60, 17), (40, 10, 90, 33)])
def test_mfma_equality_elimination_equals_numpy(shape):
    """The blocks with the n_eq equality rows eliminated (set-up kernel, second phase): Wr, UVr, (A A')r, Me, Ne and the Gram
    pivots against numpy; one to three 16-row blocks of equality rows.  The eliminated rows / columns of the reduced blocks are
    zero up to rounding and are never read."""
    from ppopt_amd import _lib
    nx, nt, nc, ne = shape
    d = _random_program(numpy.random.default_rng(nx * 1000 + nc + ne), nx, nt, nc)
    d['A'][:ne] = numpy.random.default_rng(ne).standard_normal((ne, nx))      # independent equality rows
    eng = _lib.Engine(d['A'], d['b'], d['F'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], ne)
    Qi = numpy.linalg.inv(d['Q'])
    W = d['A'] @ Qi @ d['A'].T
    UV = numpy.hstack([d['A'] @ Qi @ d['c'] + d['b'], d['A'] @ Qi @ d['H'] + d['F']])
    G = d['A'] @ d['A'].T
    E, I = numpy.arange(ne), numpy.arange(ne, nc)
    WEi, GEi = numpy.linalg.inv(W[numpy.ix_(E, E)]), numpy.linalg.inv(G[numpy.ix_(E, E)])
    cond = max(numpy.linalg.cond(d['Q']), numpy.linalg.cond(W[numpy.ix_(E, E)]), numpy.linalg.cond(G[numpy.ix_(E, E)]))
    want = {5: (W - W[:, E] @ WEi @ W[E, :])[numpy.ix_(I, I)], 6: (UV - W[:, E] @ WEi @ UV[E, :])[I],
            7: (G - G[:, E] @ GEi @ G[E, :])[numpy.ix_(I, I)], 8: WEi @ UV[E, :], 9: (WEi @ W[E, :])[:, I]}
    for which, ref in want.items():
        got = eng.program_block(which)
        assert got.size, which
        got = got[numpy.ix_(I, I)] if which in (5, 7) else (got[I] if which == 6 else (got[:, I] if which == 9 else got))
        err = numpy.max(numpy.abs(got - ref)) / (1.0 + numpy.max(numpy.abs(ref)))
        assert err <= 1e-11 * max(cond, 1.0), (shape, which, err, cond)
    gE = eng.program_block(10)
    L = numpy.linalg.cholesky(G[numpy.ix_(E, E)])
    assert numpy.allclose(gE[0], numpy.diag(L) ** 2, rtol=1e-9 * cond, atol=0) and numpy.allclose(gE[1], numpy.diag(G)[:ne], rtol=1e-13)
    eng.close()


@pytest.mark.parametrize('name', ['c2_dblint_n5', 'c2_dblint_n5_x20', 'dblint_n3'])
def test_equality_elimination_gives_the_same_solve(name, monkeypatch):
    """A/B: active sets of n_eq + (1..8) rows solved one thread per candidate on the reduced blocks (default) against the
    full (n_eq + k)-row Schur systems solved inside the theta kernel's wavefronts (MPC_NO_EQ_ELIM=1): identical verdicts on every
    level, identical region sets and index sets, coefficients within 1e-8 relative."""
    from test_gpu_parity import engine_from_golden, run_levels
    g = load_golden(name)
    nl = None if bool(g['complete']) else int(g['n_levels']) + 1
    runs = []
    for env in ({}, {'MPC_NO_EQ_ELIM': '1'}):
        with monkeypatch.context() as m:
            for key, val in env.items():
                m.setenv(key, val)
            eng = engine_from_golden(g)
            assert (eng.program_block(5).size > 0) == (not env and 'raw_Q' in g.files)
            levels, regions = run_levels(eng, nl)
            runs.append(([(c.copy(), s.copy()) for c, s, _ in levels], {tuple(r.active_set): r for r in regions}))
            eng.close()
    (la, ra), (lb, rb) = runs
    assert len(la) == len(lb)
    for (ca, sa), (cb, sb) in zip(la, lb):
        assert numpy.array_equal(ca, cb) and numpy.array_equal(sa, sb)
    assert set(ra) == set(rb)
    for key, r1 in ra.items():
        r2 = rb[key]
        assert r1.omega_set == r2.omega_set and r1.lambda_set == r2.lambda_set and r1.regular_set == r2.regular_set, key
        for fld in ('A', 'b', 'C', 'd', 'E', 'f'):
            assert rel_err(getattr(r1, fld), getattr(r2, fld)) <= COEF_TOL, (key, fld, rel_err(getattr(r1, fld), getattr(r2, fld)))


def test_mfma_setup_reports_a_semidefinite_hessian():
    """A rank-deficient Q fails the Cholesky pivot test on the device: the program runs in dense-KKT mode (no Schur blocks)."""
    from ppopt_amd import _lib
    d = _random_program(numpy.random.default_rng(3), 8, 3, 14, psd_rank=4)
    eng = _lib.Engine(d['A'], d['b'], d['F'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], 0)
    assert eng.program_block(0).size == 0 and eng.program_block(4).shape == (14, 14)
    st = (eng.pruned_clear(), eng.frontier_root(), eng.level_run(True))[2]
    assert st.kkt_mode == 1
    eng.close()


# ---- the quick test's first pass with one thread per candidate (k_xq_thread) ---------------------------------------------------------
@pytest.mark.parametrize('name', ['c4_rand_20_8_20_s0', 'c3_quadtank_n10'])
def test_thread_pass_of_the_quick_test_changes_no_verdict(name, monkeypatch):
    """k_xq_thread decides a last-level candidate by the first ratio test of the hinted column, with the arithmetic of xq_decide:
    against its generating parent's record (MPC_XQ_THREAD=1), and by default also against the records of its other parents -- any
    parent's vertex from which the missing row's slack reaches zero along one edge proves the candidate feasible.  Everything it
    leaves open goes to the wavefront kernel unchanged.  Every status of every level must be the one the wavefront kernel alone
    gives (MPC_XQ_THREAD=0), and the pass must really have decided candidates on the last level -- more with the other parents."""
    from test_gpu_parity import engine_from_golden, run_levels
    g = load_golden(name)
    nl = int(g['n_levels']) + 1
    runs = []
    for env in ({'MPC_XQ_THREAD': '0'}, {'MPC_XQ_THREAD': '1'}, {}):
        with monkeypatch.context() as m:
            m.delenv('MPC_XQ_THREAD', raising=False)
            for key, val in env.items():
                m.setenv(key, val)
            eng = engine_from_golden(g)
            levels, regions = run_levels(eng, nl)
            runs.append(([(c.copy(), s.copy(), int(st.n_children), int(st.n_xq_thread)) for c, s, st in levels], sorted(tuple(r.active_set) for r in regions)))
            eng.close()
    (la, ra), (lb, rb), (lc, rc) = runs
    assert len(la) == len(lb) == len(lc) and ra == rb == rc
    for (ca, sa, na, ta), (cb, sb, nb, tb), (cc, sc, nc_, tc) in zip(la, lb, lc):
        assert numpy.array_equal(ca, cb) and numpy.array_equal(sa, sb) and na == nb
        assert numpy.array_equal(ca, cc) and numpy.array_equal(sa, sc) and na == nc_
        assert ta == 0
    assert lb[-1][3] > 0.1 * len(lb[-1][0]), 'the thread pass decided nothing on the last level'
    assert lc[-1][3] > lb[-1][3], 'the other parents decided nothing'


# ---- one-step plans on the levels that keep dictionaries (k_xq_thread plan mode + k_x1) -----------------------------------------------
@pytest.mark.parametrize('name', ['c4_rand_20_8_20_s0', 'c3_quadtank_n10', 'c2_dblint_n5_x20'])
def test_streamed_one_step_dictionaries_equal_the_register_simplex(name, monkeypatch):
    """MPC_X1=1: a candidate whose dictionary is ONE step from its generating parent's record (column deleted / zero row pivoted /
    one Harris pivot) gets it from k_x1, which streams the record through that step, instead of k_x2's register simplex.  Same
    operations on the same numbers: every status, every child list and every region record of every level must be IDENTICAL, bit for
    bit, to MPC_X1=0.  (The default, MPC_X1=2, also starts from the candidate's other parents: other vertices of the same faces, so the
    records differ while every verdict is the reference's -- the deep goldens run with the default.)"""
    from test_gpu_parity import engine_from_golden, run_levels
    g = load_golden(name)
    nl = None if bool(g['complete']) else int(g['n_levels']) + 1
    runs = []
    for env in ({'MPC_X1': '0'}, {'MPC_X1': '1'}):
        with monkeypatch.context() as m:
            for key, val in env.items():
                m.setenv(key, val)
            eng = engine_from_golden(g)
            levels, regions = run_levels(eng, nl)
            runs.append(([(c.copy(), s.copy(), int(st.n_children)) for c, s, st in levels], {tuple(r.active_set): r for r in regions}))
            eng.close()
    (la, ra), (lb, rb) = runs
    assert len(la) == len(lb)
    for (ca, sa, na), (cb, sb, nb) in zip(la, lb):
        assert numpy.array_equal(ca, cb) and numpy.array_equal(sa, sb) and na == nb
    assert set(ra) == set(rb)
    for key, r1 in ra.items():
        r2 = rb[key]
        assert r1.omega_set == r2.omega_set and r1.lambda_set == r2.lambda_set and r1.regular_set == r2.regular_set, key
        for fld in ('A', 'b', 'C', 'd', 'E', 'f'):
            assert numpy.array_equal(getattr(r1, fld), getattr(r2, fld)), (key, fld)


@pytest.mark.parametrize('name', ['rand_6_3_12_s1', 'c2_dblint_n5', 'quadtank_n3', 'rand_5_3_8_s3', 'mplp_rand_5_3_12_s2', 'c5_control_allocation'])
def test_one_thread_pass_and_one_step_plans_forced_on_every_level(name, monkeypatch):
    """The round-5 paths take lists of >= 4,096 (thread pass) / 2,048 (plans) candidates by default, i.e. only the large levels of large
    programs.  MPC_XQT_MIN=1 MPC_X1_MIN=1 MPC_NO_SMALLPATH=1 sends EVERY level of a small program through them -- other parents, plans,
    k_x1, the pass beside the theta stage: the statuses of every level and the region set must be those of the default run (which
    the golden tests hold against the reference).  (tools/fuzz_scan.py under the same switches: 1.25 M candidates of 490 programs, no
    verdict differs from the CPU oracle, profiles/r05_fuzz_forced_paths.log.)"""
    from test_gpu_parity import engine_from_golden, run_levels
    g = load_golden(name)
    nl = None if bool(g['complete']) else int(g['n_levels']) + 1
    runs = []
    # third run: every level first runs without host round trips, reports 'repeat' and is repeated on the classic path WITH the forced
    # round-5 paths -- the repeat must not search the previous frontier for other parents (that run's children have overwritten it;
    # found in round 5 when doubtful candidates began to send small levels to the repeat); fourth: the small path in its round-4 form
    for env in ({}, {'MPC_NO_SMALLPATH': '1', 'MPC_XQT_MIN': '1', 'MPC_X1_MIN': '1'},
                {'MPC_TEST_SMALL_FALLBACK': '1', 'MPC_XQT_MIN': '1', 'MPC_X1_MIN': '1'}, {'MPC_NO_SMALL_FUSE': '1'},
                {'MPC_NO_SMALLPATH': '1', 'MPC_XQT_MIN': '1', 'MPC_X1_MIN': '1', 'MPC_NO_KKT_LISTS': '1'},
                {'MPC_NO_SMALLPATH': '1', 'MPC_XQT_MIN': '1', 'MPC_X1_MIN': '1', 'MPC_X_FIRST_MIN': '1', 'MPC_X_FIRST_MAX': '1000000000'}):      # (sixth: the (x,theta) stage queued before the region read-back on every storing level)      # (fifth: work lists by compaction instead of k_kkt_thread's own)
        with monkeypatch.context() as m:
            for key, val in env.items():
                m.setenv(key, val)
            eng = engine_from_golden(g)
            levels, regions = run_levels(eng, nl)
            runs.append(([(c.copy(), s.copy(), int(st.n_children), int(st.n_xq_thread)) for c, s, st in levels], sorted(tuple(r.active_set) for r in regions)))
            eng.close()
    la, ra = runs[0]
    for lb, rb in runs[1:]:
        assert len(la) == len(lb) and ra == rb
        for (ca, sa, na, ta), (cb, sb, nb, tb) in zip(la, lb):
            assert numpy.array_equal(ca, cb) and numpy.array_equal(sa, sb) and na == nb
    assert sum(t for *_, t in runs[1][0]) > 0, 'the forced run never used the one-thread pass'


# ---- levels without host round trips (level_run_small) and lean large levels -------------------------------------------------
@pytest.mark.parametrize('name', ['rand_6_3_12_s1', 'c2_dblint_n5', 'quadtank_n3', 'c4_rand_20_8_20_s0', 'mplp_rand_5_3_12_s2'])
def test_levels_without_host_round_trips_equal_the_classic_path(name, monkeypatch):
    """Four ways through the same levels: default (small levels keep every list length on the device, large ones most of them),
    MPC_NO_SMALLPATH=1 (every level on the classic path with its host read-backs), MPC_SMALLPATH_MAX=10^9 (every level on
    the no-round-trip path), MPC_TEST_SMALL_FALLBACK=1 (every small level runs that way, reports 'repeat', and is repeated on the
    classic path).  Same kernels, same lists: candidates, verdicts and region records must be IDENTICAL, bit for bit."""
    from test_gpu_parity import engine_from_golden, run_levels
    g = load_golden(name)
    nl = None if bool(g['complete']) else int(g['n_levels']) + 1
    runs = []
    # (fifth, round 5: the small path with the region kernel and the (x,theta) kernel as two launches instead of one grid, and its end in five launches)
    for env in ({}, {'MPC_NO_SMALLPATH': '1'}, {'MPC_SMALLPATH_MAX': '1000000000'}, {'MPC_TEST_SMALL_FALLBACK': '1'},
                {'MPC_NO_SMALL_RX': '1', 'MPC_NO_SMALL_FUSE': '1'}):
        with monkeypatch.context() as m:
            for key, val in env.items():
                m.setenv(key, val)
            eng = engine_from_golden(g)
            levels, regions = run_levels(eng, nl)
            runs.append(([(c.copy(), s.copy(), int(st.n_children)) for c, s, st in levels], {tuple(r.active_set): r for r in regions}))
            eng.close()
    la, ra = runs[0]
    for lb, rb in runs[1:]:
        assert len(la) == len(lb)
        for (ca, sa, na), (cb, sb, nb) in zip(la, lb):
            assert numpy.array_equal(ca, cb) and numpy.array_equal(sa, sb) and na == nb
        assert set(ra) == set(rb)
        for key, r1 in ra.items():
            r2 = rb[key]
            assert r1.omega_set == r2.omega_set and r1.lambda_set == r2.lambda_set and r1.regular_set == r2.regular_set, key
            for fld in ('A', 'b', 'C', 'd', 'E', 'f'):
                assert numpy.array_equal(getattr(r1, fld), getattr(r2, fld)), (key, fld)


def test_streamed_records_with_non_coherent_default(tmp_path):
    """the blocks a running kernel writes and the host polls (streamed region records, chunk flags, list lengths) are
    allocated hipHostMallocCoherent, so they do not depend on the runtime's default.  A fresh process with HIP_HOST_COHERENT=0
    solves config 4 with streaming and must return all 9,432 regions."""
    import subprocess
    import sys
    code = "\n".join(["import sys; sys.path.insert(0, '.'); import bench",
                      "from ppopt_amd.mp_solvers import mpqp_hip_combinatorial",
                      "sol = mpqp_hip_combinatorial.solve(bench.build_program('c4', 0), max_levels=5, stream=True)",
                      "print('REGIONS', len(sol.critical_regions))"])
    env = dict(os.environ, HIP_HOST_COHERENT='0')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-c', code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'REGIONS 9432' in out.stdout, out.stdout[-500:]


def test_parameter_set_without_a_vertex_is_closed_by_redundant_rows(monkeypatch):
    """The 51-region variant of config 2 (state box |x| <= 20): the presolve leaves two parallel rows of A_t, a slab without a
    vertex, and the register-resident kernels need a vertex to start their theta-space LPs from.  MPLP_Program.engine() closes the
    set with the (widened) box of theta over the whole program -- strictly redundant rows.  The solve must return exactly the
    reference's 51 regions (golden c2_dblint_n5_x20), no region may list a closing row, and it must be the solution the program gets
    without the closing rows (MPC_NO_THETA_CLOSE=1, LDS-engine kernels): same index sets, coefficients within 1e-8."""
    import warnings
    from ppopt_amd import MPQP_Program, problem_generator as pg
    from ppopt_amd.mp_solvers import mpqp_hip_combinatorial
    g = load_golden('c2_dblint_n5_x20')
    d = pg.double_integrator_data(5, 20.0)

    def build():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return MPQP_Program(d['A'], d['b'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], d['F'], equality_indices=d['equality_indices'])
    prog = build()
    assert numpy.linalg.matrix_rank(prog.A_t) < prog.num_t()          # no vertex
    eng = prog.engine(0, closed=True)
    assert eng.n_tc > eng.n_tc_program == prog.A_t.shape[0]          # closing rows were appended for the device
    assert prog.engine(0).n_tc == prog.A_t.shape[0]                  # the other drivers' handle keeps the program's own rows
    prof = []
    sol = mpqp_hip_combinatorial.solve(prog, profile=prof)
    assert sum(p.get('ms_region2', 0.0) for p in prof) > 0           # the register-resident region kernel ran
    monkeypatch.setenv('MPC_NO_THETA_CLOSE', '1')
    plain = build()
    assert plain.engine(0, closed=True).n_tc == plain.A_t.shape[0]
    ref = mpqp_hip_combinatorial.solve(plain)
    want = {tuple(int(v) for v in row[:int(kk)]) for row, kk in zip(g['R_active'], g['R_k'])}      # the reference's region active sets
    ka = {tuple(r.active_set): r for r in sol.critical_regions}
    kb = {tuple(r.active_set): r for r in ref.critical_regions}
    assert len(ka) == len(kb) == 51 and ka.keys() == kb.keys() and want == set(ka)
    for key, r1 in ka.items():
        r2 = kb[key]
        assert max(r1.omega_set, default=-1) < prog.A_t.shape[0]
        assert r1.omega_set == r2.omega_set and r1.lambda_set == r2.lambda_set and r1.regular_set == r2.regular_set, key
        for fld in ('A', 'b', 'C', 'd', 'E', 'f'):
            assert rel_err(getattr(r1, fld), getattr(r2, fld)) <= COEF_TOL, (key, fld)


def test_closing_rows_are_not_used_for_a_box_of_big_m_size():
    """A program that keeps big-M rows (right-hand sides of 1e7) has a parameter box of 1e8: closing rows that far out would ruin the
    absolute tolerances of the LPs they take part in (tools/fuzz_close.py: facet lists changed), so the handle gets the program's own rows."""
    import warnings
    from ppopt_amd import MPQP_Program, problem_generator as pg
    rng = numpy.random.default_rng(7 * 1000003 + 47)
    nx, nt, m = int(rng.integers(3, 13)), int(rng.integers(2, 7)), int(rng.integers(6, 20))
    d = pg.generate_mpqp_data(nx, nt, m, 7 * 7919 + 47)
    keep = rng.random(d['A_t'].shape[0]) < 0.5
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        prog = MPQP_Program(d['A'], d['b'], d['c'], d['H'], d['Q'], d['A_t'][keep], d['b_t'][keep], d['F'])
    assert numpy.linalg.matrix_rank(prog.A_t) < prog.num_t()
    assert prog.engine(0, closed=True).n_tc == prog.A_t.shape[0]
    prog.release_engine()


def test_config4_one_level_beyond_the_goldens_equals_the_oracle_on_a_sample(oracle):
    """Config 4 one level deeper than the benchmark and than any reference-generated golden (level 6: 5,575,526 candidates, the scaling
    workload of bench.py --gpus N): every 64th candidate's verdict and every sampled region against the CPU oracle.  The frontier of
    that level is itself a product of five levels of verdicts and prunings on the device."""
    from conftest import rel_err, rows_match
    from ppopt_amd.region_batch import RegionBatch
    from test_gpu_parity import engine_from_golden
    g = load_golden('c4_rand_20_8_20_s0')
    eng = engine_from_golden(g)
    P = oracle.problem_from_golden(g)
    eng.pruned_clear(); eng.frontier_root()
    for depth in range(6):
        st = eng.level_run(depth != 5)
        if depth != 5:
            eng.frontier_advance()
    assert int(st.n) == 5575526 and int(st.k) == 6
    cands, status = eng.frontier_get(), eng.level_status()
    hd, hi, er, kk, slots = eng.level_regions_slots()
    regs = {int(hi[j, 1]): r for j, r in zip(slots.tolist(), RegionBatch(hd, hi, er, eng.n_x, eng.n_t, eng.n_c, eng.n_tc, kk, slots).regions())}
    pick = numpy.arange(0, len(cands), 64)
    want, want_regs = P.check_level(numpy.ascontiguousarray(cands[pick]), threads=0, want_regions=True)
    got = status[pick]
    differ = numpy.nonzero(want != got)[0]
    # a differing verdict has to be knife-edge (conftest.is_knife_edge): none is expected on this program (none on levels 1-5)
    from conftest import is_knife_edge
    for j in differ.tolist():
        assert is_knife_edge(P, cands[pick[j]].tolist()), (cands[pick[j]].tolist(), int(want[j]), int(got[j]))
    assert len(differ) <= 2
    n_reg = 0
    for j, wr in want_regs.items():
        if int(got[j]) != 3:
            continue
        r = regs[int(pick[j])]
        n_reg += 1
        assert r.active_set == wr['active_set']
        assert rel_err(r.A, wr['A']) < 1e-7 and rel_err(r.b, wr['b']) < 1e-7 and rel_err(r.C, wr['C']) < 1e-7 and rel_err(r.d, wr['d']) < 1e-7
        if (r.omega_set, r.lambda_set, r.regular_set) != (wr['omega_set'], wr['lambda_set'], wr['regular_set']):
            assert is_knife_edge(P, r.active_set) or kkt_cond_large(P, r.active_set), r.active_set
        else:
            assert rows_match(r.E, r.f, wr['E'], wr['f'])
    assert n_reg > 100
    eng.close()


def kkt_cond_large(P, active_set):
    from conftest import kkt_condition
    return kkt_condition(P, active_set) > 1e6


def test_one_thread_kkt_solves_of_nine_and_ten_rows_equal_the_wavefront_solves():
    """Round 6: k_kkt_thread covers active sets of up to ten inequality rows (eight until now; deeper levels solved their KKT systems
    inside k_theta2, wavefront-wide in LDS).  generate_mpqp_data(10, 2, 20, 7) runs to cardinality 10 (its parameter set is a pointed
    cone of exactly n_theta rows: the register-resident kernels take it since round 6 as well): every level's statuses and every region
    with the one-thread solves are those with MPC_NO_KKT_THREAD=1, bit for bit -- the same operations in the same order (kkt.hpp)."""
    import subprocess
    import sys
    code = r'''
import sys, warnings, hashlib, json
sys.path.insert(0, %r)
import numpy
from ppopt_amd import MPQP_Program, problem_generator as pg
d = pg.generate_mpqp_data(10, 2, 20, 7)
with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    prog = MPQP_Program(d['A'], d['b'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], d['F'])
eng = prog.engine(0)
eng.pruned_clear(); eng.frontier_root()
out = []
depth_max = max(eng.n_x, eng.n_t) - eng.n_eq
for depth in range(depth_max):
    gen = depth + 1 != depth_max
    st = eng.level_run(gen)
    hd, hi, er, kk, slots = eng.level_regions_slots()
    regs = sorted((numpy.array(hi[j][8:8 + int(st.k)]).tobytes(), numpy.array(hd[j]).tobytes(), numpy.array(er[int(hi[j][6]):int(hi[j][6]) + int(hi[j][2])]).tobytes()) for j in slots.tolist())
    h = hashlib.sha256()
    h.update(eng.frontier_get().tobytes()); h.update(eng.level_status().tobytes())
    for r in regs:
        for piece in r: h.update(piece)
    out.append([int(st.k), int(st.n), int(st.n_regions), h.hexdigest()])
    if not gen or st.n_children == 0:
        break
    eng.frontier_advance()
print(json.dumps(out))
''' % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import json
    runs = []
    for env in ({}, {'MPC_NO_KKT_THREAD': '1'}):
        e = dict(os.environ); e.update(env)
        r = subprocess.run([sys.executable, '-c', code], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert len(runs[0]) == 10 and runs[0][-1][0] == 10
    assert runs[0] == runs[1]


def test_deferred_one_step_dictionaries_change_nothing(monkeypatch):
    """Round 6: on a storing level k_x1 runs on its own stream beside the end of the level and the next level's KKT kernel, and is joined by
    the first kernel that reads a dictionary record (MPC_X1_DEFER, default on, only without per-kernel event timing).  Config 4 to its
    fifth level and config 3 to its fourth: the regions with and without the deferral are the same objects, bit for bit."""
    import bench
    from ppopt_amd.mp_solvers import mpqp_hip_combinatorial
    for wl in ('c4', 'c3'):
        sols = []
        for defer in ('1', '0'):
            monkeypatch.setenv('MPC_X1_DEFER', defer)
            prog = bench.build_program(wl)
            sols.append(mpqp_hip_combinatorial.solve(prog, max_levels=bench.WORKLOADS[wl][2]))      # (no profile: the deferral is active)
            prog.release_engine()
        a, b = sols
        assert len(a.critical_regions) == len(b.critical_regions) > 100
        for r1, r2 in zip(a.critical_regions, b.critical_regions):
            assert list(r1.active_set) == list(r2.active_set)
            assert r1.omega_set == r2.omega_set and r1.lambda_set == r2.lambda_set and r1.regular_set == r2.regular_set
            for fld in ('A', 'b', 'C', 'd', 'E', 'f'):
                assert numpy.asarray(getattr(r1, fld)).tobytes() == numpy.asarray(getattr(r2, fld)).tobytes(), (wl, fld)


def test_children_from_the_bucketed_pruned_list_equal_the_full_scan(monkeypatch):
    """Round 6: on a level whose children stage is large (parents x pruned sets >= MPC_PRUNED_BUCKET_MIN) a parent scans only the pruned sets
    whose smallest non-equality member is one of its own members (k_children_count_b over a list bucketed at the level's start) instead of
    the whole list.  Config 4 to level 4 (three levels of children) and a program with an equality row: the children of every level -- hence
    the frontiers -- are identical with the bucketed scan forced onto every level and with the full scan."""
    from test_gpu_parity import engine_from_golden
    for name, n_levels in (('c4_rand_20_8_20_s0', 4), ('c2_dblint_n5', 5), ('quadtank_n3', 5)):
        g = load_golden(name)
        runs = []
        for env in ('1', '0'):
            monkeypatch.setenv('MPC_PRUNED_BUCKET_MIN', env)      # 1: every level with a pruned set; 0: never
            monkeypatch.setenv('MPC_PRUNED_BUCKET_NP', '1')
            monkeypatch.setenv('MPC_NO_SMALLPATH', '1')            # (the bucketed scan lives on the classic path)
            eng = engine_from_golden(g)
            eng.pruned_clear(); eng.frontier_root()
            fr = []
            for depth in range(n_levels):
                st = eng.level_run(True)
                fr.append((eng.level_children().copy(), eng.level_status().copy()))
                if st.n_children == 0:
                    break
                eng.frontier_advance()
            eng.close()
            runs.append(fr)
        assert len(runs[0]) == len(runs[1]) >= 3
        for (c1, s1), (c2, s2) in zip(*runs):
            assert numpy.array_equal(s1, s2) and numpy.array_equal(c1, c2), name


def test_small_level_kkt_lanes_and_helper_workgroups_change_nothing(monkeypatch):
    """Round 6: on a small level k_kkt_thread gives a candidate eight lanes -- each repeats the factorisation, the box screen's rows are
    dealt among them, the verdict is the OR (MPC_KKT_SPREAD=0: one lane) -- and lists its own output instead of a compaction launch
    (MPC_NO_KKT_LISTS=1).  Every level's statuses and children, and every region of configs 4 and 2, are the same either way."""
    import bench
    from ppopt_amd.mp_solvers import mpqp_hip_combinatorial
    from test_gpu_parity import engine_from_golden
    new = {'MPC_KKT_SPREAD': '1', 'MPC_NO_KKT_LISTS': '0', 'MPC_KKT_BOX_SELECT': '0'}
    old = {'MPC_KKT_SPREAD': '0', 'MPC_NO_KKT_LISTS': '1', 'MPC_KKT_BOX_SELECT': '1'}      # (the last: the screen's row test with selects instead of max(a blo, a bhi))
    for name, n_levels in (('c4_rand_20_8_20_s0', 4), ('c2_dblint_n5', 5), ('quadtank_n3', 5), ('c3_quadtank_n10', 3)):
        g = load_golden(name)
        runs = []
        for env in (new, old):
            for kk, vv in env.items():
                monkeypatch.setenv(kk, vv)
            eng = engine_from_golden(g)
            eng.pruned_clear(); eng.frontier_root()
            fr = []
            for depth in range(n_levels):
                st = eng.level_run(True)
                fr.append((eng.level_children().copy(), eng.level_status().copy(), st.n_regions))
                if st.n_children == 0:
                    break
                eng.frontier_advance()
            eng.close()
            runs.append(fr)
        assert len(runs[0]) == len(runs[1]) >= 2
        for (c1, s1, r1), (c2, s2, r2) in zip(*runs):
            assert numpy.array_equal(s1, s2) and numpy.array_equal(c1, c2) and r1 == r2, name
    for wl in ('c4', 'c2'):
        sols = []
        for env in (new, old):
            for kk, vv in env.items():
                monkeypatch.setenv(kk, vv)
            prog = bench.build_program(wl)
            sols.append(mpqp_hip_combinatorial.solve(prog, max_levels=bench.WORKLOADS[wl][2]))
            prog.release_engine()
        a, b = sols
        assert len(a.critical_regions) == len(b.critical_regions) > 3
        for r1, r2 in zip(a.critical_regions, b.critical_regions):
            assert list(r1.active_set) == list(r2.active_set)
            for fld in ('A', 'b', 'C', 'd', 'E', 'f'):
                assert numpy.asarray(getattr(r1, fld)).tobytes() == numpy.asarray(getattr(r2, fld)).tobytes(), (wl, fld)


def test_doubtful_cached_runs_repeated_inside_the_kernel_give_the_lds_engines_verdicts(monkeypatch):
    """Round 6: k_x2 repeats a doubtful run from a cached record at once from the program's own dictionary (MPC_X_SECOND_MAX repeats per
    level; a fresh run decides up to growth MPC_X_FRESH_LIMIT) instead of leaving it to the LDS engine behind the level.  Config 3 -- the
    configuration with such candidates, 217 on its last level -- and a random program: every level's statuses and children with the
    repeats and the fresh-run rule switched off (everything doubtful goes to the LDS engine, rounds 2-5) and on."""
    from test_gpu_parity import engine_from_golden
    for name, n_levels in (('c3_quadtank_n10', 4), ('c4_rand_20_8_20_s0', 4), ('big_24_7_34_s430912', 3)):
        g = load_golden(name)
        runs = []
        for second, fresh in (('1024', '1e6'), ('0', '0')):
            monkeypatch.setenv('MPC_X_SECOND_MAX', second)
            monkeypatch.setenv('MPC_X_FRESH_LIMIT', fresh)
            eng = engine_from_golden(g)
            eng.pruned_clear(); eng.frontier_root()
            fr = []
            for depth in range(n_levels):
                st = eng.level_run(True)
                fr.append((eng.level_children().copy(), eng.level_status().copy(), st.n_regions))
                if st.n_children == 0:
                    break
                eng.frontier_advance()
            eng.close()
            runs.append(fr)
        assert len(runs[0]) == len(runs[1]) >= 2
        for (c1, s1, r1), (c2, s2, r2) in zip(*runs):
            assert numpy.array_equal(s1, s2) and numpy.array_equal(c1, c2) and r1 == r2, name
