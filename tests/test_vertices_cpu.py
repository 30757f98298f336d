"""Vertex enumeration and the recursive-feasibility certificate without a device: the independent references against known
vertex sets, every refusal raised before any device call, the host assembly of the closed-loop maps and box corners, and the margin-LP
rows of a small hand program."""
import numpy
import pytest

import vertex_reference as ref
from ppopt_amd import _lib, invariance
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.geometry.polytope import Polytope
from ppopt_amd.geometry.vertices import polytope_vertices, vertices_of_rows
from ppopt_amd.solution import Solution


# ---- the references against known vertex sets -------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', range(2, 9))
def test_reference_cube(n):
    A, b, V = ref.cube(n)
    assert ref.same_set(ref.qhull(A, b), V)
    if n <= 5:
        assert ref.same_set(ref.brute_force(A, b), V)


@pytest.mark.parametrize('n', range(2, 7))
def test_reference_simplex(n):
    A, b, V = ref.simplex(n)
    assert ref.same_set(ref.brute_force(A, b), V)
    assert ref.same_set(ref.qhull(A, b), V)


@pytest.mark.parametrize('n', range(3, 7))
def test_reference_cross_polytope(n):
    A, b, V = ref.cross_polytope(n)
    assert ref.same_set(ref.qhull(A, b), V)
    if n <= 4:
        assert ref.same_set(ref.brute_force(A, b), V)


def test_reference_cyclic_polytope():
    A, b, V = ref.cyclic_polytope(4, 9)
    assert ref.same_set(ref.qhull(A, b), V)
    assert ref.same_set(ref.brute_force(A, b), V)


# ---- refusals, before any device call --------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the device was called')
    monkeypatch.setattr(_lib, 'region_vertices', boom)
    monkeypatch.setattr(_lib, 'lp_solve_batch', boom)


def test_vertices_refusals(no_device):
    A, b, _ = ref.cube(3)
    with pytest.raises(ValueError, match='n_theta'):
        polytope_vertices(Polytope(numpy.ones((2, 17)), numpy.ones(2)))
    with pytest.raises(ValueError, match='more than 256'):
        polytope_vertices(Polytope(numpy.ones((257, 2)), numpy.ones(257)))
    with pytest.raises(ValueError, match='finite'):
        polytope_vertices(Polytope(A, numpy.r_[b[:-1], numpy.inf]))
    with pytest.raises(ValueError, match='finite'):
        polytope_vertices(Polytope(numpy.where(A == 1, numpy.nan, A), b))
    with pytest.raises(ValueError, match='budget'):
        polytope_vertices(Polytope(A, b), budget=1000)
    with pytest.raises(ValueError, match='slab'):
        polytope_vertices(Polytope(A, b), slab=4)
    with pytest.raises(ValueError, match='tol'):
        polytope_vertices(Polytope(A, b), tol=-1.0)
    with pytest.raises(ValueError, match='n_theta'):
        vertices_of_rows([0, 2], numpy.ones((2, 1)), 0)


class _Prog:
    """the 1-D program of tests/test_gpu_recursive_feasibility.py: x = u, |u| <= 1, |a theta + u| <= c_max, |theta| <= T"""
    def __init__(self, a=2.0, c_max=0.5, T=10.0):
        self.A = numpy.array([[1.0], [-1.0], [1.0], [-1.0]])
        self.b = numpy.array([1.0, 1.0, c_max, c_max])
        self.F = numpy.array([[0.0], [0.0], [-a], [a]])
        self.A_t = numpy.array([[1.0], [-1.0]])
        self.b_t = numpy.array([T, T])
        self.equality_indices = []

    def num_t(self):
        return 1


def _solution(n_t=1, y_fixation=None):
    E = numpy.vstack([numpy.eye(n_t), -numpy.eye(n_t)])
    r = CriticalRegion(A=numpy.zeros((1, n_t)), b=numpy.zeros((1, 1)), C=None, d=None, E=E, f=numpy.ones((2 * n_t, 1)), active_set=[],
                       omega_set=[], lambda_set=[], regular_set=[])
    if y_fixation is not None:
        r.y_fixation, r.x_indices, r.y_indices = y_fixation, [0], [1]
    P = _Prog()
    if n_t != 1:
        P.num_t = lambda: n_t
    return Solution(P, [r])


def test_certificate_refusals(no_device):
    s = _solution()
    A, B = numpy.array([[2.0]]), numpy.array([[1.0]])
    with pytest.raises(ValueError, match='mixed-integer'):
        _solution(y_fixation=numpy.array([1.0])).certify_recursive_feasibility(A, B, [0])
    with pytest.raises(ValueError, match='A must be'):
        s.certify_recursive_feasibility(numpy.eye(2), B, [0])
    with pytest.raises(ValueError, match='B must be'):
        s.certify_recursive_feasibility(A, numpy.ones((2, 1)), [0])
    with pytest.raises(ValueError, match='inputs'):
        s.certify_recursive_feasibility(A, B, [0, 0])
    with pytest.raises(ValueError, match='out of range'):
        s.certify_recursive_feasibility(A, B, [3])
    with pytest.raises(ValueError, match='finite'):
        s.certify_recursive_feasibility(numpy.array([[numpy.nan]]), B, [0])
    with pytest.raises(ValueError, match='finite'):
        s.certify_recursive_feasibility(A, B, [0], c=[numpy.inf])
    with pytest.raises(ValueError, match='lo <= hi'):
        s.certify_recursive_feasibility(A, B, [0], disturbance=([0.1], [-0.1]))
    with pytest.raises(ValueError, match='finite'):
        s.certify_recursive_feasibility(A, B, [0], disturbance=([-numpy.inf], [0.1]))
    s11 = _solution(11)
    with pytest.raises(ValueError, match='n_theta <= 10'):
        s11.certify_recursive_feasibility(numpy.eye(11), numpy.ones((11, 1)), [0], disturbance=(-numpy.ones(11), numpy.ones(11)))


# ---- host assembly ------------------------------------------------------------------------------------------------------------------
def test_closed_loop_maps_by_hand():
    # two regions of a 2-D law with three rows; inputs [2, 0]
    xlaw = numpy.zeros((2, 3, 3))
    xlaw[0, 0] = [1.0, 2.0, 3.0]
    xlaw[0, 2] = [-1.0, 0.5, 0.0]
    xlaw[1, 0] = [0.0, 1.0, 0.0]
    xlaw[1, 2] = [2.0, 0.0, -1.0]
    A = numpy.array([[1.0, 1.0], [0.0, 1.0]])
    B = numpy.array([[1.0, 0.0], [0.0, 2.0]])
    c = numpy.array([0.5, -0.5])
    Phi, phi = invariance.closed_loop_maps(xlaw, A, B, numpy.array([2, 0]), c)
    # region 0: u0 = -1 + 0.5 t0, u1 = 1 + 2 t0 + 3 t1
    assert numpy.allclose(Phi[0], [[1.5, 1.0], [4.0, 7.0]]) and numpy.allclose(phi[0], [-0.5, 1.5])
    # region 1: u0 = 2 - t1, u1 = t0
    assert numpy.allclose(Phi[1], [[1.0, 0.0], [2.0, 1.0]]) and numpy.allclose(phi[1], [2.5, -0.5])
    pts, vert = invariance.image_points(numpy.array([[1.0, 0.0], [0.0, 1.0]]), numpy.array([0, 1]), Phi, phi)
    assert numpy.allclose(pts, [[1.0, 5.5], [2.5, 0.5]]) and vert.tolist() == [0, 1]
    corners = invariance.box_corners([-1.0, -2.0], [1.0, 2.0])
    assert corners.tolist() == [[-1.0, -2.0], [1.0, -2.0], [-1.0, 2.0], [1.0, 2.0]]
    pts, vert = invariance.image_points(numpy.array([[1.0, 0.0]]), numpy.array([0]), Phi, phi, box=([-1.0, -2.0], [1.0, 2.0]))
    assert numpy.allclose(pts, [[0.0, 3.5], [2.0, 3.5], [0.0, 7.5], [2.0, 7.5]]) and vert.tolist() == [0, 0, 0, 0]


def test_margin_lp_rows_by_hand():
    P = _Prog(a=2.0, c_max=0.5, T=10.0)
    A3, b2, eq, c = invariance.margin_lp_rows(P, numpy.array([[0.25]]))
    # rows: u <= 1, -u <= 1, u <= 0.5 - 2 theta, -u <= 0.5 + 2 theta, theta <= 10, -theta <= 10, -s <= 1
    rhs = numpy.array([1.0, 1.0, 0.0, 1.0])
    assert numpy.allclose(b2[0], [1.0, 1.0, 0.0, 1.0, 9.75, 10.25, 1.0])
    assert numpy.allclose(A3[0, :, 0], [1.0, -1.0, 1.0, -1.0, 0.0, 0.0, 0.0])
    assert numpy.allclose(A3[0, :, 1], numpy.r_[-(1 + numpy.abs(rhs)), -11.0, -11.0, -1.0])
    assert eq.tolist() == [0] * 7 and c.tolist() == [0.0, 1.0]
    P.equality_indices = [0]
    A3, _, eq, _ = invariance.margin_lp_rows(P, numpy.array([[0.25]]))
    assert eq.tolist() == [1, 0, 0, 0, 0, 0, 0] and A3[0, 0, 1] == 0.0
