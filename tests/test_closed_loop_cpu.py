"""Closed-loop simulation without a device: argument validation before any device call, the box disturbance against an
independent Philox replay, the plant helpers against the programs' prediction matrices, the C ABI's stats struct, and the host reference
loop on a hand-built 1-D piecewise-affine controller with a hand-computed trajectory.  The exact reference on stacked rows
(closed_loop_reference.simulate_rows) is held against the same hand computation and against the host loop, and every case of
tests/closed_loop_cases.py, which the device tests run, has to be exact and to exercise what it is there for."""
import ctypes
import os
import subprocess
import tempfile

import numpy
import pytest

import closed_loop_cases as cases
import closed_loop_reference as ref
import hit_and_run_reference as hr
from ppopt_amd import _lib, closed_loop, problem_generator as pg
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.solution import Solution

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Prog:
    def __init__(self, n_t):
        self.n_t = n_t

    def num_t(self):
        return self.n_t


def _interval(lo, hi, slope, offset):
    """the region lo <= theta <= hi of one parameter with the law x = slope theta + offset"""
    return CriticalRegion(numpy.array([[slope]]), numpy.array([[offset]]), numpy.zeros((0, 1)), numpy.zeros((0, 1)),
                          numpy.array([[-1.0], [1.0]]), numpy.array([[-lo], [hi]]), [])


def pwa_1d(tol=1e-5):
    """u = 1 on [-2, -1], u = -theta / 2 on [-1, 1], u = -1 on [1, 2]"""
    regs = [_interval(-2.0, -1.0, 0.0, 1.0), _interval(-1.0, 1.0, -0.5, 0.0), _interval(1.0, 2.0, 0.0, -1.0)]
    return Solution(_Prog(1), regs, point_location_tolerance=tol)


def as_rows(sol):
    """(row_off, ef, xlaw) of a Solution: rows [f | E], laws [b | A], in list order"""
    regs = sol.critical_regions
    off = numpy.cumsum([0] + [len(cr.E) for cr in regs])
    ef = numpy.vstack([numpy.c_[cr.f.reshape(-1, 1), cr.E] for cr in regs])
    return off, ef, numpy.array([numpy.c_[cr.b.reshape(-1, 1), cr.A] for cr in regs])


def test_host_reference_gives_the_hand_computed_trajectory():
    sol = pwa_1d()
    A, B = [[1.0]], [[1.0]]
    out = ref.simulate(sol, [[-2.0], [1.75], [2.5]], 4, A, B, [0])
    # from -2: region 0 (u = 1) twice -- -1 lies in region 0 within the tolerance and region 0 comes first -- then region 1 at 0
    numpy.testing.assert_array_equal(out['theta'][0, :, 0], [-2.0, -1.0, 0.0, 0.0, 0.0])
    numpy.testing.assert_array_equal(out['region'][0], [0, 0, 1, 1])
    numpy.testing.assert_array_equal(out['u'][0, :, 0], [1.0, 1.0, 0.0, 0.0])
    # from 1.75: u = -1, then halving in region 1
    numpy.testing.assert_array_equal(out['theta'][1, :, 0], [1.75, 0.75, 0.375, 0.1875, 0.09375])
    numpy.testing.assert_array_equal(out['region'][1], [2, 1, 1, 1])
    assert out['status'].tolist() == [0, 0, 2] and out['exit_step'].tolist() == [4, 4, 0]
    # outside every region at once: nothing recorded after theta_0
    assert out['theta'][2, 0, 0] == 2.5 and numpy.isnan(out['theta'][2, 1:]).all() and (out['region'][2] == -1).all()
    # stop_tol = 0: steady at the first repeated state
    st = ref.simulate(sol, [[-2.0]], 6, A, B, [0], stop_tol=0.0)
    assert st['status'].tolist() == [1] and st['exit_step'].tolist() == [3]
    assert numpy.isnan(st['theta'][0, 4:]).all()
    # c and w enter after the B terms
    cw = ref.simulate(sol, [[1.75]], 1, A, B, [0], c=[0.25], w=numpy.full((1, 1, 1), 0.125))
    assert cw['theta'][0, 1, 0] == 0.25 + 1.75 - 1.0 + 0.125


def test_exact_reference_gives_the_hand_computed_trajectory():
    """the trajectories of test_host_reference_gives_the_hand_computed_trajectory from the rows alone, with a lattice tolerance"""
    row_off, ef, xlaw = as_rows(pwa_1d())
    tol = 2.0 ** -10
    A, B = [[1.0]], [[1.0]]
    out = ref.simulate_rows(row_off, ef, xlaw, [[-2.0], [1.75], [2.5]], 4, A, B, [0], tol=tol)
    numpy.testing.assert_array_equal(out['theta'][0, :, 0], [-2.0, -1.0, 0.0, 0.0, 0.0])
    numpy.testing.assert_array_equal(out['region'][0], [0, 0, 1, 1])
    numpy.testing.assert_array_equal(out['u'][0, :, 0], [1.0, 1.0, 0.0, 0.0])
    numpy.testing.assert_array_equal(out['theta'][1, :, 0], [1.75, 0.75, 0.375, 0.1875, 0.09375])
    numpy.testing.assert_array_equal(out['region'][1], [2, 1, 1, 1])
    assert out['status'].tolist() == [0, 0, 2] and out['exit_step'].tolist() == [4, 4, 0]
    assert out['theta'][2, 0, 0] == 2.5 and numpy.isnan(out['theta'][2, 1:]).all() and (out['region'][2] == -1).all()
    assert numpy.isnan(out['u'][2]).all()
    assert out['traj_steps'] == 4 + 4 + 1     # the step that finds no region counts
    # 0.09375 = 3 / 32 is the finest number met: 3 / 32 against +-2 needs six bits, and the row tests with tol = 2^-10 eleven more
    assert 6 <= out['bits'] <= 17
    st = ref.simulate_rows(row_off, ef, xlaw, [[-2.0]], 6, A, B, [0], tol=tol, stop_tol=0.0)
    assert st['status'].tolist() == [1] and st['exit_step'].tolist() == [3] and st['traj_steps'] == 3
    assert numpy.isnan(st['theta'][0, 4:]).all() and st['theta'][0, 3, 0] == 0.0
    cw = ref.simulate_rows(row_off, ef, xlaw, [[1.75]], 1, A, B, [0], c=[0.25], w=numpy.full((1, 1, 1), 0.125), tol=tol)
    assert cw['theta'][0, 1, 0] == 0.25 + 1.75 - 1.0 + 0.125
    # exactly tol beyond the last row: outside by the strict rule, inside by the inclusive one; and a non-finite start
    edge = ref.simulate_rows(row_off, ef, xlaw, [[2.0 + tol], [numpy.inf]], 1, A, B, [0], tol=tol)
    assert edge['status'].tolist() == [2, 3] and edge['exit_step'].tolist() == [0, 0] and edge['traj_steps'] == 1
    assert ref.simulate_rows(row_off, ef, xlaw, [[2.0 + tol]], 1, A, B, [0], tol=tol, inclusive=True)['region'].tolist() == [[2]]
    # a number that is no float64 is refused, not rounded: 1 + 2^-60
    with pytest.raises(AssertionError):
        ref.simulate_rows(row_off, ef, xlaw, [[1.0]], 1, [[2.0 ** -60]], B, [0], c=[1.5], tol=tol)


def test_exact_reference_agrees_with_the_host_loop():
    """two regions of two parameters with a law in R^3, wrapped as rows: on lattice data the float64 loop rounds nothing either, so
    the two references have to agree in every field, NaN tails included"""
    tol = 2.0 ** -10
    sol = _sol2(tol)
    rng = numpy.random.default_rng(5)
    n, steps = 60, 5
    theta0 = ref.lattice_starts(rng, n, 2, tol, reach=1.25, edge=1.0)
    A, B, c = numpy.array([[0.5, 0.25], [-0.25, 0.75]]), numpy.array([[0.25, 0.0, -0.5], [0.0, 0.5, 0.25]]), numpy.array([0.25, -0.5])
    w = ref.lattice_disturbance(rng, n, steps, 2)
    for kw in (dict(), dict(c=c), dict(w=w), dict(c=c, w=w, stop_tol=0.25)):
        want = ref.simulate(sol, theta0, steps, A, B, [2, 0, 2], **kw)
        got = ref.simulate_rows(*as_rows(sol), theta0, steps, A, B, [2, 0, 2], tol=tol, **kw)
        for key in ('theta', 'u', 'region', 'status', 'exit_step'):
            assert numpy.array_equal(got[key], want[key], equal_nan=True), (kw.keys(), key)
        assert set(want['status']) >= {0, 2} and (want['region'] == 1).any() and (want['region'] == 0).any()
    assert set(want['status']) == {0, 1, 2}


def test_the_exact_cases_cover_every_width():
    """both edges of every theta width with both input widths, every input count of the issue, every combination of c and w, a stop
    tolerance at every theta width, n_x above n_u, and inputs that are neither sorted nor distinct"""
    seen = {(cases.case(name)['n_t'], cases.case(name)['n_u']) for name in cases.WIDTH_CASES}
    assert {n_t for n_t, _ in seen} == {1, 4, 5, 8, 9, 16} and {n_u for _, n_u in seen} == {1, 4, 5, 16}
    width = lambda n_t: 4 if n_t <= 4 else 8 if n_t <= 8 else 16
    assert {(width(n_t), n_u <= 4) for n_t, n_u in seen} == {(wd, small) for wd in (4, 8, 16) for small in (False, True)}
    for n_t in (1, 4, 5, 8, 9, 16):
        assert len({n_u for t, n_u in seen if t == n_t}) == 2
    ks = [cases.case(name) for name in cases.WIDTH_CASES]
    assert {(k['c'] is not None, k['w'] is not None) for k in ks} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {width(k['n_t']) for k in ks if k['stop_tol'] is not None} == {4, 8, 16}
    for k in ks:
        assert k['n_x'] in (17, 20) and k['n_x'] > k['n_u'] and len(k['inputs']) == k['n_u'] and max(k['inputs']) < k['n_x']
        if k['n_u'] >= 2:
            assert len(set(k['inputs'])) < k['n_u'] and k['inputs'] != sorted(k['inputs'])
        # the two adjacency tables describe the same cells: ids across bits 63 / 64, and in words 2 and 3
        m2, m4 = k['walk2'][0], k['walk4'][0]
        assert m2.shape[1] == 2 and m4.shape[1] == 4 and m2[:, 0].any() and m2[:, 1].any() and m4[:, 2].any() and m4[:, 3].any()
    assert {cases.case(name)['n_t'] for name in cases.RULES_CASES} == {4, 9}


@pytest.mark.parametrize('name', cases.LATTICE_CASES)
def test_every_exact_case_is_exact_and_exercises_the_kernel(name):
    """conditions on the inputs, shown by the reference alone: the certificate (at most 53 bits), a fifth of the trajectories run every
    step, five or more lose their region at a step >= 1, a steady end wherever a stop tolerance is set, the region changes in a
    quarter of the consecutive step pairs, and in some block of 256 trajectories three different exit steps occur while another
    trajectory runs on (the barrier-synchronised continuation of the scan)"""
    k, out = cases.case(name), cases.expected(name)
    q = cases.quality(out, k['steps'])
    print(name, q)
    assert q['bits'] <= 53
    assert q['full'] >= 0.2 and q['lost_later'] >= 5 and q['lost_at_start'] >= 1 and q['changes'] >= 0.25 and q['staggered'] >= 3
    assert (q['steady'] >= 1) == (k['stop_tol'] is not None)
    assert q['regions'] >= 0.8 * sum(1 for r in range(len(k['row_off']) - 1) if k['row_off'][r + 1] > k['row_off'][r])
    if k['flags'].get('overlapping'):
        assert k['steps'] >= 2


def test_replay_step_is_the_documented_order():
    rng = numpy.random.default_rng(3)
    th, u = rng.normal(size=(50, 3)), rng.normal(size=(50, 2))
    A, B, c, w = rng.normal(size=(3, 3)), rng.normal(size=(3, 2)), rng.normal(size=3), rng.normal(size=(50, 3))
    got = closed_loop.replay_step(th, u, A, B, c, w)
    for p in range(50):
        for i in range(3):
            v = c[i]
            for j in range(3):
                v = v + A[i, j] * th[p, j]
            for l in range(2):
                v = v + B[i, l] * u[p, l]
            assert got[p, i] == v + w[p, i]


@pytest.mark.parametrize('seed,n_t', [(0, 1), (7, 4), ((123 << 32) + 99, 5), (2 ** 64 - 1, 16)])
def test_disturbance_box_is_philox_bit_for_bit(seed, n_t):
    n, steps = 37, 11
    rng = numpy.random.default_rng(n_t)
    lo = rng.uniform(-2, 0, size=n_t)
    hi = lo + rng.uniform(0, 3, size=n_t)
    got = closed_loop.disturbance_box(seed, n, steps, lo, hi)
    k0, k1 = seed & 0xffffffff, ((seed >> 32) ^ 0x636c6f6f) & 0xffffffff
    want = numpy.empty((n, steps, n_t))
    for p in range(n):
        for k in range(steps):
            for j in range((n_t + 1) // 2):
                r = [int(v) for v in hr.philox4x32_10(p & 0xffffffff, p >> 32, k, j, k0, k1)]
                for i, (a, b) in ((2 * j, (r[0], r[1])), (2 * j + 1, (r[2], r[3]))):
                    if i < n_t:
                        want[p, k, i] = lo[i] + (hi[i] - lo[i]) * float(hr.u53(a, b))
    assert numpy.array_equal(got.view(numpy.uint64), want.view(numpy.uint64))
    assert numpy.all((got >= lo) & (got <= hi))


def test_plant_helpers_match_the_programs():
    d2 = pg.double_integrator_data(5)
    p2 = pg.double_integrator_plant(5)
    assert numpy.array_equal(d2['F'][0:2], p2['A'])                 # F_eq[0:2] = A
    assert numpy.array_equal(d2['A'][0:2, p2['inputs']], -p2['B'])   # the u_0 column of A_eq is -B
    assert numpy.all(d2['A'][2:10, p2['inputs']] == 0)
    d3 = pg.quad_tank_data(10)
    p3 = pg.quad_tank_plant()
    N, nu, nx = 10, 2, 4
    Phi = d3['F'][2 * nu * N + nx * N:2 * nu * N + nx * N + nx]       # the rows +Phi of F
    Gam = d3['A'][2 * nu * N:2 * nu * N + nx]                        # the rows +Gam of A
    assert numpy.array_equal(Phi, p3['A'])                           # Phi[0:4] = A
    assert numpy.array_equal(Gam[:, 0:2], p3['B'])                   # Gam[0:4, 0:2] = B
    assert p3['inputs'] == [0, 1]


def test_sim_stats_layout_matches_header():
    fields = [name for name, *_ in _lib.SimStats._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mpcombi.h"\nint main(void) {\n  printf("%zu\\n", sizeof(mpc_sim_stats));\n' + \
           ''.join(f'  printf("{f} %zu\\n", offsetof(mpc_sim_stats, {f}));\n' for f in fields) + \
           '  printf("MPC_SIM_FINAL %d\\n", MPC_SIM_FINAL);\n  printf("MPC_SIM_KEY_SALT %d\\n", MPC_SIM_KEY_SALT);\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, 's.c'), os.path.join(tmp, 's')
        open(src, 'w').write(prog)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), src, '-o', exe])
        out = subprocess.check_output([exe]).decode().split('\n')
    assert int(out[0]) == ctypes.sizeof(_lib.SimStats)
    vals = dict((line.split()[0], int(line.split()[1])) for line in out[1:] if line.strip())
    for f in fields:
        assert vals[f] == getattr(_lib.SimStats, f).offset, f
    assert vals['MPC_SIM_FINAL'] == _lib.MPC_SIM_FINAL and vals['MPC_SIM_KEY_SALT'] == _lib.MPC_SIM_KEY_SALT
    assert _lib.MPC_SIM_FINAL not in (_lib.MPC_LOCATE_OVERLAPPING, _lib.MPC_LOCATE_INCLUSIVE, _lib.MPC_LOCATE_WALK, _lib.MPC_LOCATE_TREE)
    assert 'mpc_locator_simulate' in _lib.EXPORTED_SYMBOLS


def _no_device(monkeypatch):
    def boom(self, device=0):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(Solution, 'locator', boom)


def _sol2(tol=1e-5):
    """two regions of two parameters, law x in R^3"""
    regs = []
    for s in (1.0, -1.0):
        E = numpy.array([[s, 0.0], [0.0, 1.0], [0.0, -1.0], [-s, 0.0]])
        regs.append(CriticalRegion(numpy.ones((3, 2)), numpy.zeros((3, 1)), numpy.zeros((0, 2)), numpy.zeros((0, 1)), E,
                                   numpy.array([[1.0], [1.0], [1.0], [0.0]]), []))
    return Solution(_Prog(2), regs, point_location_tolerance=tol)


BAD = [
    (dict(theta0=[[0.0, 0.0, 0.0]]), 'theta0 must be'),
    (dict(theta0=[[numpy.nan, 0.0]]), 'theta0 must be finite'),
    (dict(A=numpy.eye(3)), 'A must be'),
    (dict(A=[[1.0, numpy.inf], [0.0, 1.0]]), 'A must be finite'),
    (dict(B=numpy.ones((3, 1))), 'B must be'),
    (dict(B=[[numpy.nan], [1.0]]), 'B must be finite'),
    (dict(inputs=[3]), 'out of range'),
    (dict(inputs=[-1]), 'out of range'),
    (dict(inputs=[0, 1]), 'integer indices'),
    (dict(B=numpy.ones((2, 17)), inputs=list(range(17))), 'n_u = 17'),
    (dict(c=[0.0, numpy.nan]), 'c must be finite'),
    (dict(c=[0.0]), 'c must have'),
    (dict(disturbance=([0.0, 0.0], [1.0])), 'two vectors'),
    (dict(disturbance=([0.0, 1.0], [1.0, 0.0])), 'lo <= hi'),
    (dict(disturbance=([0.0, numpy.nan], [1.0, 1.0])), 'box must be finite'),
    (dict(disturbance=numpy.zeros((1, 4, 2))), 'disturbance array must be'),
    (dict(disturbance=numpy.full((1, 3, 2), numpy.inf)), 'disturbance must be finite'),
    (dict(steps=0), 'steps must be'),
    (dict(steps=2.5), 'steps must be'),
    (dict(seed=-1), 'seed must be'),
    (dict(stop_tol=-1.0), 'stop_tol'),
    (dict(stop_tol=numpy.nan), 'stop_tol'),
    (dict(locate='bsp'), 'locate must be'),
    (dict(record='some'), 'record must be'),
    (dict(locate='walk'), 'walk needs'),
]


@pytest.mark.parametrize('kw,msg', BAD, ids=[m for _, m in BAD])
def test_bad_arguments_raise_before_any_device_call(monkeypatch, kw, msg):
    _no_device(monkeypatch)
    args = dict(theta0=[[0.5, 0.0]], steps=3, A=numpy.eye(2), B=numpy.ones((2, 1)), inputs=[2])
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        _sol2().simulate(**args)


def test_theta_dimension_and_budget_are_refused_before_any_device_call(monkeypatch):
    _no_device(monkeypatch)
    n = 17
    regs = [CriticalRegion(numpy.ones((1, n)), numpy.zeros((1, 1)), numpy.zeros((0, n)), numpy.zeros((0, 1)), numpy.eye(n),
                           numpy.ones((n, 1)), [])]
    with pytest.raises(ValueError, match='n_theta = 17'):
        Solution(_Prog(n), regs).simulate(numpy.zeros((1, n)), 2, numpy.eye(n), numpy.ones((n, 1)), [0])
    with pytest.raises(ValueError, match='budget'):
        _sol2().simulate(numpy.zeros((1_000_000, 2)), 1000, numpy.eye(2), numpy.ones((2, 1)), [0])
    with pytest.raises(ValueError, match='no region'):
        Solution(_Prog(2), []).simulate([[0.0, 0.0]], 2, numpy.eye(2), numpy.ones((2, 1)), [0])
