"""Search trees without a device: trees built by the independent CPU reference (tests/search_tree_reference.py) on
hand-built solutions, checked for their structure, for host descent equal to a numpy re-statement of the scan, and through the
C++ / JavaScript export."""
import hashlib
import os
import shutil
import subprocess

import numpy
import pytest

import search_tree_reference as ref
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.solution import Solution
from ppopt_amd.upop import SearchTree
from ppopt_amd.upop.linear_code_gen import generate_code_cpp, generate_code_js, plane_table

TOL = 1e-5


class _Prog:
    def __init__(self, n_x, n_t, rng, quadratic=True):
        self.c = rng.normal(size=(n_x, 1))
        self.H = rng.normal(size=(n_x, n_t))
        if quadratic:
            M = rng.normal(size=(n_x, n_x))
            self.Q = M @ M.T + numpy.eye(n_x)
        self.c_c = numpy.zeros((1, 1))
        self.c_t = numpy.zeros((n_t, 1))
        self.Q_t = numpy.zeros((n_t, n_t))
        self._nt = n_t

    def num_t(self):
        return self._nt

    def evaluate_objective(self, x, th):
        v = th.T @ self.H.T @ x + self.c.T @ x
        if hasattr(self, 'Q'):
            v = v + 0.5 * x.T @ self.Q @ x
        return float(v[0, 0])


def _region(E, f, rng, n_x=2):
    E = numpy.asarray(E, float)
    n_t = E.shape[1]
    return CriticalRegion(rng.normal(size=(n_x, n_t)), rng.normal(size=(n_x, 1)), numpy.zeros((0, n_t)), numpy.zeros((0, 1)), E,
                          numpy.asarray(f, float).reshape(-1, 1), [])


def _triangles(rng, scale=1.0, centre=(0.0, 0.0), row_scales=None):
    """the box [-1, 1]^2 (scaled, shifted) cut by its diagonals into four triangles"""
    cx, cy = centre
    tri = [([[0, 1], [1, -1], [-1, -1]], [1, 0, 0]), ([[1, 0], [-1, 1], [-1, -1]], [1, 0, 0]),
           ([[0, -1], [-1, 1], [1, 1]], [1, 0, 0]), ([[-1, 0], [1, -1], [1, 1]], [1, 0, 0])]
    regs = []
    for k, (E, f) in enumerate(tri):
        E = numpy.array(E, float)
        f = numpy.array(f, float) * scale + E @ numpy.array([cx, cy])
        if row_scales is not None:
            s = numpy.array(row_scales[k % len(row_scales)], float)
            E, f = E * s[:, None], f * s
        regs.append(_region(E, f, rng))
    return regs


def cases():
    rng = numpy.random.default_rng(3)
    out = {}
    out['triangles'] = Solution(_Prog(2, 2, rng), _triangles(rng), point_location_tolerance=TOL)
    out['scaled'] = Solution(_Prog(2, 2, rng), _triangles(rng, row_scales=[[1e3, 1.0, 1e-3], [0.5, 20.0, 1.0]]), point_location_tolerance=TOL)
    tiny = _triangles(rng, scale=1e-4, centre=(0.3, -0.2))
    far = _triangles(rng, scale=2.0, centre=(1e5, -3e4))
    out['tiny_far'] = Solution(_Prog(2, 2, rng), _triangles(rng) + tiny + far, point_location_tolerance=TOL)
    unb = [_region([[-1.0, 0.0]], [-1.0], rng), _region([[1.0, 0.0], [0.0, 1.0]], [1.0, 0.0], rng), _region([[1.0, 0.0], [0.0, -1.0]], [1.0, 0.0], rng)]
    out['unbounded'] = Solution(_Prog(2, 2, rng), unb, point_location_tolerance=TOL)
    boxes = []
    for k in range(6):   # overlapping boxes
        lo = rng.uniform(-1, 0.5, size=2)
        hi = lo + rng.uniform(0.3, 1.0, size=2)
        boxes.append(_region(numpy.vstack([numpy.eye(2), -numpy.eye(2)]), numpy.r_[hi, -lo], rng))
    out['overlapping'] = Solution(_Prog(2, 2, rng), boxes, is_overlapping=True, point_location_tolerance=TOL)
    # three parameters: a simplex split by a hyperplane
    E3 = [[[-1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [0, -1, -1]], [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 1, 1], [0, -1, -1]]]
    out['three'] = Solution(_Prog(2, 3, rng), [_region(E, [0, 1, 1, 1, 1], rng) for E in E3], point_location_tolerance=TOL)
    return out


CASES = cases()


def reference_tree(sol, band=None, leaf_size=1, max_depth=48):
    ef, row_off, xlaw = sol._stacked()
    planes, start, plane_of, _ = plane_table(sol.critical_regions, sol.theta_dim())
    band = 16 * sol.point_location_tolerance if band is None else band
    return ref.build(ef, row_off, planes, start, plane_of, sol.point_location_tolerance, band, leaf_size, max_depth)


_TREES = {}


def tree_of(name, band=None):
    if (name, band) not in _TREES:
        _TREES[name, band] = reference_tree(CASES[name], band)
    return _TREES[name, band]


def sample_points(sol, arrays, rng, n=400):
    ef, row_off, _ = sol._stacked()
    pts = [rng.uniform(-2.5, 2.5, size=(n, sol.theta_dim()))]
    for cr in sol.critical_regions:   # around every region, also far ones and tiny ones
        c = ref._centre(numpy.hstack([cr.f.reshape(-1, 1), cr.E]))
        pts.append(c + rng.normal(size=(20, sol.theta_dim())) * (1e-3 + 1e-6 * numpy.abs(c).max()))
    pts.append(ref.near_split_points(arrays, ef, row_off, sol.point_location_tolerance, rng, per=2))
    pts.append(rng.uniform(50, 100, size=(10, sol.theta_dim())))   # outside Theta
    return numpy.vstack(pts)


@pytest.mark.parametrize('name', sorted(CASES))
def test_structure(name):
    sol = CASES[name]
    t = tree_of(name)
    plus, minus, lo, hi, _ = t['classification']
    N = len(t['node_plane'])
    off, items = t['node_off'], t['items']
    for k in range(N):
        lst = items[off[k]:off[k + 1]]
        assert numpy.all(numpy.diff(lst) > 0), 'leaf lists ascend'
    sets = [None] * N
    for k in reversed(range(N)):
        if t['node_plane'][k] < 0:
            sets[k] = set(items[off[k]:off[k + 1]].tolist())
        else:
            assert all(c > k for c in t['node_child'][k])
            sets[k] = sets[t['node_child'][k][0]] | sets[t['node_child'][k][1]]
    assert sets[0] == set(range(len(sol.critical_regions)))
    for k in range(N):
        h = t['node_plane'][k]
        if h < 0:
            continue
        cp, cm = (sets[c] for c in t['node_child'][k])
        for j in sets[k] - cp:   # absent from the "+" subtree: "-" only, and tau+ covers it
            assert minus[j, h] and not plus[j, h] and max(0.0, hi[j, h]) <= t['node_tau'][k, 1]
        for j in sets[k] - cm:
            assert plus[j, h] and not minus[j, h] and max(0.0, -lo[j, h]) <= t['node_tau'][k, 0]


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_descent_equals_the_scan(name):
    sol = CASES[name]
    arrays = tree_of(name)
    tree = SearchTree.from_arrays(sol, arrays)
    assert tree.depth() >= 1
    ef, row_off, xlaw = sol._stacked()
    P = sol.program
    pts = sample_points(sol, arrays, numpy.random.default_rng(11))
    for inclusive in (False, True):
        for tol in (TOL, 0.5 * TOL, 0.0):
            if tol == 0.0 and not inclusive:
                continue
            for th in pts:
                want = ref.scan(ef, row_off, xlaw, th, tol, sol.is_overlapping, inclusive, getattr(P, 'Q', None), P.c, P.H)
                assert tree.locate(th, inclusive=inclusive, tol=tol) == want, (name, th, inclusive, tol)
    with pytest.raises(ValueError):
        tree.locate(pts[0], tol=2 * TOL)


@pytest.mark.parametrize('name', ['triangles', 'tiny_far', 'overlapping'])
def test_band_zero_and_large_band_agree(name):
    sol = CASES[name]
    ef, row_off, xlaw = sol._stacked()
    a0 = SearchTree.from_arrays(sol, tree_of(name, 0.0))
    a1 = SearchTree.from_arrays(sol, tree_of(name, 0.1))
    for th in sample_points(sol, tree_of(name), numpy.random.default_rng(5), n=300):
        assert a0.locate(th) == a1.locate(th) == ref.scan(ef, row_off, xlaw, th, TOL, sol.is_overlapping, False,
                                                         getattr(sol.program, 'Q', None), sol.program.c, sol.program.H)


# sha256 of the tree-less exports of CASES['triangles'] / ['overlapping'] as the code generator wrote them before search trees
EXPORT_SHA = {('triangles', 'cpp'): '52353445ab4ec018a0f1a498a37e89daf77d7753d19251d3803b78f79a4469ab', ('triangles', 'js'): '7fd0e9a36c03420446dba272ebfa048bc87ed09971ba2a29f99337dc5f3606a2',
              ('overlapping', 'cpp'): 'ab45a2aa75aeab848b4a04f095e97d4295383e6c25aa8988a08d6643c78e3f74', ('overlapping', 'js'): 'a68ee4ddd83d803df5e966273872d2adf9c713e2bd2820908e0a0294503079a2'}


@pytest.mark.parametrize('name', ['triangles', 'overlapping'])
def test_treeless_exports_unchanged(name):
    sol = CASES[name]
    assert hashlib.sha256(generate_code_cpp(sol, 'double').encode()).hexdigest() == EXPORT_SHA[name, 'cpp']
    assert hashlib.sha256(generate_code_js(sol).encode()).hexdigest() == EXPORT_SHA[name, 'js']


_DRIVER = r'''
#include <cstdio>
#include "solution.hpp"
int main() {
    double th[%(n)d];
    while (true) {
        for (int t = 0; t < %(n)d; ++t) if (std::scanf("%%lf", &th[t]) != 1) return 0;
        std::printf("%%d\n", ppopt_solution::locate(th));
    }
}
'''


def _run_cpp(src, n, pts, tmp, tag):
    d = os.path.join(tmp, tag)
    os.makedirs(d)
    with open(os.path.join(d, 'solution.hpp'), 'w') as fh:
        fh.write(src)
    with open(os.path.join(d, 'main.cpp'), 'w') as fh:
        fh.write(_DRIVER % {'n': n})
    subprocess.check_call(['g++', '-std=c++11', '-Wall', '-Werror', '-O1', os.path.join(d, 'main.cpp'), '-o', os.path.join(d, 'main')])
    inp = '\n'.join(' '.join(repr(float(v)) for v in p) for p in pts) + '\n'
    out = subprocess.run([os.path.join(d, 'main')], input=inp, capture_output=True, text=True, check=True).stdout
    return numpy.array(out.split(), dtype=int)


def _run_js(src, pts, tmp, tag):
    path = os.path.join(tmp, tag + '.js')
    with open(path, 'w') as fh:
        fh.write(src + '\nconst pts = JSON.parse(require("fs").readFileSync(0, "utf8"));\n'
                 'console.log(JSON.stringify(pts.map(p => locate(p))));\n')
    import json
    out = subprocess.run(['node', path], input=json.dumps(pts.tolist()), capture_output=True, text=True, check=True).stdout
    return numpy.array(json.loads(out), dtype=int)


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
@pytest.mark.parametrize('name', sorted(CASES))
def test_tree_export_cpp_equals_treeless(name, tmp_path):
    sol = CASES[name]
    tree = SearchTree.from_arrays(sol, tree_of(name))
    pts = sample_points(sol, tree_of(name), numpy.random.default_rng(2))
    plain = _run_cpp(generate_code_cpp(sol, 'double'), sol.theta_dim(), pts, str(tmp_path), 'plain')
    treed = _run_cpp(generate_code_cpp(sol, 'double', tree=tree), sol.theta_dim(), pts, str(tmp_path), 'tree')
    assert numpy.array_equal(plain, treed)
    assert (plain >= 0).any()


@pytest.mark.skipif(shutil.which('node') is None, reason='needs node')
@pytest.mark.parametrize('name', sorted(CASES))
def test_tree_export_js_equals_treeless(name, tmp_path):
    sol = CASES[name]
    tree = SearchTree.from_arrays(sol, tree_of(name))
    pts = sample_points(sol, tree_of(name), numpy.random.default_rng(4))
    assert numpy.array_equal(_run_js(generate_code_js(sol), pts, str(tmp_path), 'plain'),
                             _run_js(generate_code_js(sol, tree=tree), pts, str(tmp_path), 'tree'))


def test_to_arrays_round_trip():
    sol = CASES['tiny_far']
    tree = SearchTree.from_arrays(sol, tree_of('tiny_far'))
    again = SearchTree.from_arrays(sol, tree.to_arrays())
    for k in ('planes', 'node_plane', 'node_child', 'node_tau', 'node_off', 'items'):
        assert numpy.array_equal(getattr(tree, k), getattr(again, k))
    assert again.tol == tree.tol
