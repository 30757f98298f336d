"""Merging regions with equal laws without a device: the independent CPU reference (tests/region_merge_reference.py) on
hand-built solutions with known answers, the host assembly of a merged solution (location, evaluation, C++ export) and every
refusal of Solution.merge_regions."""
import shutil
import subprocess

import numpy
import pytest

import region_merge_reference as ref
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.region_merge import MergedRegion, build_merged_solution
from ppopt_amd.solution import Solution
from ppopt_amd.upop.linear_code_gen import generate_code_cpp


class _Prog:
    """the little of a program that a merged solution reads"""

    def __init__(self, n_t):
        self._nt = n_t

    def num_t(self):
        return self._nt


def _box_rows(lo, hi):
    n = len(lo)
    E = numpy.vstack([numpy.eye(n), -numpy.eye(n)])
    return E, numpy.concatenate([numpy.asarray(hi, float), -numpy.asarray(lo, float)])


def _region(E, f, A, b):
    E = numpy.asarray(E, float)
    n_t = E.shape[1]
    return CriticalRegion(numpy.asarray(A, float).reshape(-1, n_t), numpy.asarray(b, float).reshape(-1, 1), numpy.zeros((0, n_t)),
                          numpy.zeros((0, 1)), E, numpy.asarray(f, float).reshape(-1, 1), [0])


LAW_A = numpy.array([[1.0, -2.0], [0.5, 0.25]])
LAW_B = numpy.array([[3.0], [-1.0]])


def _sol(regions, n_t=2):
    s = Solution(_Prog(n_t), regions, point_location_tolerance=1e-5)
    s.is_complete = True
    return s


def triangles():
    """the square [-1, 1]^2 cut by its diagonals into four triangles, one law"""
    tri = [([[0, 1], [1, -1], [-1, -1]], [1, 0, 0]), ([[1, 0], [-1, 1], [-1, -1]], [1, 0, 0]),
           ([[0, -1], [-1, 1], [1, 1]], [1, 0, 0]), ([[-1, 0], [1, -1], [1, 1]], [1, 0, 0])]
    return _sol([_region(E, f, LAW_A, LAW_B) for E, f in tri])


def ell():
    """an L of three unit squares: [0,1]^2, [1,2]x[0,1], [0,1]x[1,2]"""
    return _sol([_region(*_box_rows(lo, hi), LAW_A, LAW_B) for lo, hi in (((0, 0), (1, 1)), ((1, 0), (2, 1)), ((0, 1), (1, 2)))])


def gap():
    return _sol([_region(*_box_rows(lo, hi), LAW_A, LAW_B) for lo, hi in (((0, 0), (1, 1)), ((1.5, 0), (2.5, 1)))])


def two_laws():
    """adjacent squares whose laws share row 0 only"""
    A2 = LAW_A.copy()
    A2[1, 0] += 1.0
    return _sol([_region(*_box_rows((0, 0), (1, 1)), LAW_A, LAW_B), _region(*_box_rows((1, 0), (2, 1)), A2, LAW_B)])


def near_laws(delta):
    """adjacent squares whose laws differ by delta (1 + max |[A | b]|) in one entry"""
    A2 = LAW_A.copy()
    A2[0, 1] += delta * (1.0 + numpy.max(numpy.abs(numpy.hstack([LAW_A, LAW_B]))))
    return _sol([_region(*_box_rows((0, 0), (1, 1)), LAW_A, LAW_B), _region(*_box_rows((1, 0), (2, 1)), A2, LAW_B)])


def chain():
    """1-D intervals [k, k + 1], k = 0..4"""
    return _sol([_region([[1.0], [-1.0]], [k + 1.0, -float(k)], [[2.0]], [1.0]) for k in range(5)], n_t=1)


def slabs():
    """[0, 1]^3 cut into four slabs across x_0"""
    cuts = [0.0, 0.25, 0.5, 0.75, 1.0]
    A = numpy.array([[1.0, 0.0, -1.0]])
    return _sol([_region(*_box_rows((cuts[k], 0, 0), (cuts[k + 1], 1, 1)), A, [0.5]) for k in range(4)], n_t=3)


def half_strips():
    """two unbounded half-strips {0 <= y <= 1, x <= 0} and {0 <= y <= 1, x >= 0}, and a bounded square away from both (another law)"""
    E = [[0, 1], [0, -1], [1, 0]]
    regs = [_region(E, [1, 0, 0], LAW_A, LAW_B), _region([[0, 1], [0, -1], [-1, 0]], [1, 0, 0], LAW_A, LAW_B),
            _region(*_box_rows((0, 3), (1, 4)), LAW_A + 1.0, LAW_B)]
    return _sol(regs)


# name -> (solution builder, outputs, expected member lists)
CASES = {
    'triangles': (triangles, None, [[0, 1, 2, 3]]),
    'ell': (ell, None, [[0, 1], [2]]),
    'gap': (gap, None, [[0], [1]]),
    'two_laws_all_rows': (two_laws, None, [[0], [1]]),
    'two_laws_shared_row': (two_laws, [0], [[0, 1]]),
    'laws_within_half_tol': (lambda: near_laws(0.5e-8), None, [[0, 1]]),
    'laws_twice_the_tol': (lambda: near_laws(2e-8), None, [[0], [1]]),
    'chain_1d': (chain, None, [[0, 1, 2, 3, 4]]),
    'slabs_3d': (slabs, None, [[0, 1, 2, 3]]),
    'half_strips': (half_strips, None, [[0, 1], [2]]),
}


def _canonical(E, f):
    """unit rows [n | o] sorted lexicographically"""
    E = numpy.asarray(E, float)
    f = numpy.asarray(f, float).reshape(-1)
    n = numpy.linalg.norm(E, axis=1)
    rows = numpy.column_stack([E / n[:, None], f / n])
    return rows[numpy.lexsort(rows.T[::-1])]


@pytest.mark.parametrize('name', sorted(CASES))
def test_reference_merges_as_expected(name):
    build, outputs, want = CASES[name]
    src = build()
    merged, info = ref.merge_reference(src, outputs)
    assert merged.merge_info['members'] == want
    assert [r.members for r in merged.critical_regions] == want
    assert all(isinstance(r, MergedRegion) for r in merged.critical_regions)
    assert info['knife'] == 0
    n_t = src.theta_dim()
    outs = list(range(numpy.asarray(src.critical_regions[0].A).reshape(-1, n_t).shape[0])) if outputs is None else outputs
    for r in merged.critical_regions:
        first = src.critical_regions[r.members[0]]
        numpy.testing.assert_array_equal(r.A, numpy.asarray(first.A).reshape(-1, n_t)[outs])
        numpy.testing.assert_array_equal(r.b, numpy.asarray(first.b).reshape(-1, 1)[outs])
        assert r.C.shape == (0, n_t) and r.d.shape == (0, 1) and r.active_set == []
        if len(r.members) == 1:
            numpy.testing.assert_array_equal(r.E, first.E)
            numpy.testing.assert_array_equal(r.f, first.f)
        else:
            numpy.testing.assert_allclose(numpy.linalg.norm(r.E, axis=1), 1.0, rtol=0, atol=1e-12)
    assert src.merge_info is None and merged.is_overlapping is False


def test_merged_geometry_of_the_hand_built_cases():
    sq = ref.merge_reference(triangles())[0].critical_regions[0]
    numpy.testing.assert_allclose(_canonical(sq.E, sq.f), _canonical(*_box_rows((-1, -1), (1, 1))), atol=1e-12)
    iv = ref.merge_reference(chain())[0].critical_regions[0]
    numpy.testing.assert_allclose(_canonical(iv.E, iv.f), _canonical([[1.0], [-1.0]], [5.0, 0.0]), atol=1e-12)
    bx = ref.merge_reference(slabs())[0].critical_regions[0]
    numpy.testing.assert_allclose(_canonical(bx.E, bx.f), _canonical(*_box_rows((0, 0, 0), (1, 1, 1))), atol=1e-12)
    st = ref.merge_reference(half_strips())[0].critical_regions[0]
    numpy.testing.assert_allclose(_canonical(st.E, st.f), _canonical([[0, 1], [0, -1]], [1, 0]), atol=1e-12)


def test_reference_pair_test():
    assert not ref.pair_rejected(_box_rows((0, 0), (1, 1)), _box_rows((1, 0), (2, 1)))
    assert ref.pair_rejected(_box_rows((0, 0), (1, 1)), _box_rows((1, 0.5), (2, 1.5)))     # a step: not convex


def _host_points(sol, rng, n=4000):
    lo = numpy.full(sol.theta_dim(), -1.5)
    hi = numpy.full(sol.theta_dim(), 2.5)
    return rng.uniform(lo, hi, size=(n, sol.theta_dim()))


@pytest.mark.parametrize('name', ['triangles', 'ell', 'two_laws_shared_row', 'slabs_3d'])
def test_built_solution_locates_and_evaluates_on_the_host(name):
    build, outputs, want = CASES[name]
    src = build()
    merged, _ = ref.merge_reference(src, outputs)
    n_t = src.theta_dim()
    outs = list(range(numpy.asarray(src.critical_regions[0].A).reshape(-1, n_t).shape[0])) if outputs is None else outputs
    rng = numpy.random.default_rng(3)
    hits = 0
    for th in _host_points(src, rng, 1500):
        th = th.reshape(-1, 1)
        r = src.get_region(th)
        k = merged.get_region(th)
        if r is None:
            # outside every source region by more than the location tolerance: outside every merged region too
            if all(numpy.max(numpy.asarray(c.E) @ th - numpy.asarray(c.f)) > 1e-4 for c in src.critical_regions):
                assert k is None
            continue
        assert k is not None
        hits += 1
        i = src.critical_regions.index(r)
        slack = -numpy.max(numpy.asarray(r.E) @ th - numpy.asarray(r.f))
        if slack >= 1e-6:
            assert any(c.is_inside(th, 1e-5) for c in (src.critical_regions[m] for m in k.members))
            if i in k.members:
                numpy.testing.assert_allclose(merged.evaluate(th), r.evaluate(th)[outs], rtol=1e-12, atol=1e-12)
    assert hits >= 10


def test_build_merged_solution_checks_the_partition():
    src = ell()
    with pytest.raises(ValueError, match='partition'):
        build_merged_solution(src, [[0], [1]], [None, None], [0, 1])
    with pytest.raises(ValueError, match='one member'):
        build_merged_solution(src, [[0, 1], [2]], [None, None], [0, 1])
    m = build_merged_solution(src, [[2], [1, 0]], [None, numpy.column_stack([[1.0, 0.0, 2.0, 0.0], [[0, 1], [0, -1], [1, 0], [-1, 0]]])], [1])
    assert [r.members for r in m.critical_regions] == [[0, 1], [2]]
    assert m.merge_info['outputs'] == [1] and m.merge_info['source'] is src
    assert m.critical_regions[0].A.shape == (1, 2)


MAIN = r'''
#include <cstdio>
#include "solution.hpp"
int main() {
    using namespace ppopt_solution;
    double theta[64], x[256];
    for (;;) {
        for (int t = 0; t < n_theta; ++t) if (std::scanf("%lf", &theta[t]) != 1) return 0;
        const int r = locate(theta);
        std::printf("%d", r);
        if (evaluate(theta, x)) for (int i = 0; i < n_x; ++i) std::printf(" %.17g", x[i]);
        std::printf("\n");
    }
}
'''


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
@pytest.mark.parametrize('name', ['triangles', 'ell', 'two_laws_shared_row'])
def test_generated_cpp_of_a_merged_solution(name, tmp_path):
    build, outputs, _ = CASES[name]
    merged, _ = ref.merge_reference(build(), outputs)
    (tmp_path / 'solution.hpp').write_text(generate_code_cpp(merged, float_type='double'))
    (tmp_path / 'main.cpp').write_text(MAIN)
    exe = str(tmp_path / 'a.out')
    subprocess.check_call(['g++', '-O1', '-std=c++11', '-Wall', '-Werror', str(tmp_path / 'main.cpp'), '-o', exe])
    pts = _host_points(merged, numpy.random.default_rng(5), 500)
    feed = '\n'.join(' '.join(repr(float(v)) for v in th) for th in pts) + '\n'
    out = subprocess.run([exe], input=feed, capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert len(out) == len(pts)
    hits = 0
    for line, th in zip(out, pts):
        tok = line.split()
        cr = merged.get_region(th.reshape(-1, 1))
        want = -1 if cr is None else merged.critical_regions.index(cr)
        assert int(tok[0]) == want
        if want >= 0:
            hits += 1
            numpy.testing.assert_allclose([float(v) for v in tok[1:]], merged.evaluate(th.reshape(-1, 1)).ravel(), rtol=1e-12, atol=1e-12)
    assert hits > 50


def test_refusals():
    src = ell()
    over = ell()
    over.is_overlapping = True
    with pytest.raises(ValueError, match='overlapping'):
        over.merge_regions()
    mi = ell()
    mi.critical_regions[0].y_fixation = numpy.array([1.0])
    mi.critical_regions[0].x_indices = [0, 1]
    mi.critical_regions[0].y_indices = [2]
    with pytest.raises(ValueError, match='mixed-integer'):
        mi.merge_regions()
    big = _sol([_region(*_box_rows(numpy.zeros(17), numpy.ones(17)), numpy.ones((1, 17)), [0.0])], n_t=17)
    with pytest.raises(ValueError, match='n_theta = 17'):
        big.merge_regions()
    rows = _sol([_region(numpy.tile([[1.0, 0.0]], (257, 1)), numpy.ones(257), LAW_A, LAW_B)])
    with pytest.raises(ValueError, match='more than 256 rows'):
        rows.merge_regions()
    for bad in ([2], [-1], [], [0, 5]):
        with pytest.raises(ValueError, match='outputs'):
            src.merge_regions(outputs=bad)
    with pytest.raises(ValueError, match='tol'):
        src.merge_regions(tol=-1.0)


def test_merged_solution_refuses_what_needs_the_full_law():
    from ppopt_amd.upop.upop_payload import payload_cpp, payload_js, save_matlab
    src = ell()
    merged, _ = ref.merge_reference(src)
    th = numpy.array([[0.5], [0.5]])
    for call in (lambda: merged.evaluate_objective(th), lambda: merged.verify_solution(), lambda: merged.verify_theta(th),
                 lambda: merged.kkt_residuals(merged.critical_regions[0], th), lambda: merged.sample_check()):
        with pytest.raises(ValueError, match='source'):
            call()
    for call in (lambda: payload_cpp(merged), lambda: payload_js(merged), lambda: save_matlab(merged, '/nonexistent/x.mat')):
        with pytest.raises(ValueError, match='merged'):
            call()
