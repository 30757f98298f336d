"""The region stage of a small level beside the NEXT level's kernels (mpc_solve_start's loop; DESIGN 6j, csrc/mpcombi_hip.hip RegionDefer).

Every test goes through the public ``solve()`` without a profile (a profile switches the HIP-event records on, and with them the
deferral off) and compares with the same solve whose small levels build their regions in line: ``mpc_set_region_overlap(h, 2)``.  The
library's environment table is pinned by tests/test_knobs_cpu.py, so the switch is the handle's existing one, not a new variable:
1 = default, 2 = small levels in line, 3 = the first deferred level closed on the handle reports a miss.  What a level did is read from
its statistics after the solve (``Engine.solve_level_wait``): ``region_side_stream`` is 2 for a level closed one level late and 3 for the
in-line repeat of a level whose launch missed."""
import warnings

import numpy
import pytest

from conftest import golden_regions, load_golden

pytestmark = pytest.mark.gpu

DEFAULT, IN_LINE, FORCED_MISS = 1, 2, 3


def make_program(name, mode):
    from test_host_logic import build_program
    from ppopt_amd import Solver
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        prog = build_program(load_golden(name), Solver())
    eng = prog.engine(0, closed=True)
    assert eng._L.mpc_set_region_overlap(eng._h, mode) == 0
    return prog, eng


def solve_once(prog, eng, max_levels, profile=None):
    """-> ({active set: region}, number of regions listed, per level (n, n_regions, n_children, status histogram), per level region_side_stream)
    ``profile``: a list switches the handle's timing on for this solve (``mpc_set_timing``), as every solve that asks for a profile does."""
    from ppopt_amd.mp_solvers import mpqp_hip_combinatorial as m
    sol = m.solve(prog, max_levels=max_levels, profile=profile)
    regions = list(sol.critical_regions)
    levels, codes = [], []
    for lv in range(eng.solve_wait()):
        st, _ = eng.solve_level_wait(lv)
        levels.append((int(st.n), int(st.n_regions), int(st.n_children), [int(v) for v in st.n_status]))
        codes.append(int(st.region_side_stream))
    print(f'levels (n, regions, children): {[l[:3] for l in levels]}  region_side_stream: {codes}')
    return {tuple(r.active_set): r for r in regions}, len(regions), levels, codes


def assert_same(got, want):
    (ra, na, la, _), (rb, nb, lb, _) = got, want
    assert la == lb
    assert na == len(ra) and nb == len(rb), 'a region is listed twice'
    assert nb > 0 and set(ra) == set(rb)
    for key, r1 in ra.items():
        r2 = rb[key]
        assert r1.omega_set == r2.omega_set and r1.lambda_set == r2.lambda_set and r1.regular_set == r2.regular_set, key
        for fld in ('A', 'b', 'C', 'd', 'E', 'f'):
            assert numpy.array_equal(getattr(r1, fld), getattr(r2, fld)), (key, fld)


def in_line(name, max_levels):
    prog, eng = make_program(name, IN_LINE)
    want = solve_once(prog, eng, max_levels)
    assert 2 not in want[3] and 3 not in want[3]
    return want


@pytest.mark.parametrize('name,max_levels', [('c2_dblint_n5', None), ('c2_dblint_n5_x20', None), ('rand_6_3_12_s1', None), ('c4_rand_20_8_20_s0', 3)])
def test_same_solution_and_the_deferral_took_place(name, max_levels):
    """Regions bit for bit, per-level candidates / regions / children / status histogram; at least one level was closed one level late.
    c4 with three levels: its last level (15,691 candidates) runs on the classic path and joins the launch of the small level before."""
    want = in_line(name, max_levels)
    prog, eng = make_program(name, DEFAULT)
    got = solve_once(prog, eng, max_levels)
    assert_same(got, want)
    assert got[3].count(2) >= 1 and 3 not in got[3]
    assert got[3][-1] != 2, 'the last level has no level after it'
    if name.startswith('c4'):
        assert got[2][-1][0] > 4096 and got[3][-2] == 2      # a classic level behind a deferring one


def test_a_small_path_level_with_many_candidates_joins(monkeypatch):
    """MPC_SMALLPATH_MAX=10^9: the 15,691-candidate level of c4 runs without host round trips and waits for the launch before its k_children_write"""
    monkeypatch.setenv('MPC_SMALLPATH_MAX', '1000000000')
    want = in_line('c4_rand_20_8_20_s0', 3)
    prog, eng = make_program('c4_rand_20_8_20_s0', DEFAULT)
    got = solve_once(prog, eng, 3)
    assert_same(got, want)
    assert got[3][-2] == 2 and got[2][-1][0] > 4096


def test_forced_miss_restarts_the_solve():
    """The first close reports a miss: one abandoned pass, the level repeated in line (3), nothing deferred afterwards (the handle's flag is
    sticky), the same solution with every region once."""
    want = in_line('c2_dblint_n5_x20', None)
    prog, eng = make_program('c2_dblint_n5_x20', FORCED_MISS)
    got = solve_once(prog, eng, None)
    assert_same(got, want)
    assert got[3].count(3) == 1 and 2 not in got[3]
    again = solve_once(prog, eng, None)
    assert_same(again, want)
    assert 2 not in again[3] and 3 not in again[3]


def test_real_miss_on_the_degenerate_program():
    """c5_control_allocation has optimal candidates with lower-dimensional regions: the pass that meets one is abandoned, the solution is
    that of the in-line solve, and the handle's second solve defers nothing."""
    want = in_line('c5_control_allocation', None)
    prog, eng = make_program('c5_control_allocation', DEFAULT)
    got = solve_once(prog, eng, None)
    assert_same(got, want)
    assert got[3].count(3) == 1, 'no deferred launch met a lower-dimensional region'
    again = solve_once(prog, eng, None)
    assert_same(again, want)
    assert 2 not in again[3] and 3 not in again[3]


def test_the_levels_own_fallback_discards_its_launch(monkeypatch):
    """MPC_TEST_SMALL_FALLBACK=1: every small level reports 'repeat on the classic path' after its launches -- a deferring level waits for
    its own region launch, drops it and is repeated in line.  No level is closed late, and the handle solves again the same way."""
    monkeypatch.setenv('MPC_TEST_SMALL_FALLBACK', '1')
    want = in_line('c2_dblint_n5_x20', None)
    prog, eng = make_program('c2_dblint_n5_x20', DEFAULT)
    got = solve_once(prog, eng, None)
    assert_same(got, want)
    assert 2 not in got[3] and 3 not in got[3]
    assert_same(solve_once(prog, eng, None), want)


def test_two_solves_back_to_back_on_one_handle():
    """the first solution released before the second solve: the two buffer sets are back where they were, the same levels defer again
    (c2: no level of it meets a doubtful candidate, which would send the handle to the small path's unfused form for good)"""
    want = in_line('c2_dblint_n5', None)
    prog, eng = make_program('c2_dblint_n5', DEFAULT)
    first = solve_once(prog, eng, None)
    assert_same(first, want)
    codes = first[3]
    levels = first[2]
    del first
    second = solve_once(prog, eng, None)
    assert_same(second, want)
    assert second[3] == codes and second[2] == levels and codes.count(2) >= 1


# ---- two terms of the deferral's gate (SmallRun::begin, csrc/level_small.hpp): the fused form only, and never under the handle's timing ----
GATE_GOLDENS = ['c2_dblint_n5', 'rand_6_3_12_s1']


def assert_nothing_deferred(name, got):
    """no level closed late or repeated after a miss; the in-line solve's regions bit for bit; the active sets the reference recorded"""
    assert 2 not in got[3] and 3 not in got[3]
    assert_same(got, in_line(name, None))
    assert sorted(got[0]) == sorted(golden_regions(load_golden(name)))


@pytest.mark.parametrize('name', GATE_GOLDENS)
def test_the_round_4_form_defers_nothing(name, monkeypatch):
    """MPC_NO_SMALL_FUSE=1 in default mode: a small level that re-solves its doubtful candidates in place builds its regions in line"""
    monkeypatch.setenv('MPC_NO_SMALL_FUSE', '1')
    prog, eng = make_program(name, DEFAULT)
    assert_nothing_deferred(name, solve_once(prog, eng, None))


@pytest.mark.parametrize('name', GATE_GOLDENS)
def test_timing_defers_nothing(name):
    """the handle's timing switched on (a solve with a profile) in default mode: the per-stage events are recorded in line, no level defers"""
    prog, eng = make_program(name, DEFAULT)
    profile = []
    got = solve_once(prog, eng, None, profile=profile)
    assert eng._timing is True and len(profile) > 0
    assert_nothing_deferred(name, got)
