"""Slices without a device: the scipy reference of tests/slice_reference.py on hand-made polygons, the argument checks of
Solution.slice_2d / slice_1d and of _lib.slice_polygons / slice_intervals (all raise before any launch), and the drawing of a
synthetic SolutionSlice with the Agg backend."""
import numpy
import pytest

import slice_reference as ref
from ppopt_amd import Solution, _lib
from ppopt_amd.geometry import Polytope, SolutionSlice, slice_polytopes

BOX = numpy.array([-3.0, -3.0, 3.0, 3.0])
I2, Z2 = numpy.eye(2), numpy.zeros(2)


def test_reference_square():
    E = numpy.array([[1.0, 0], [0, 1], [-1, 0], [0, -1]])
    out = ref.slice_polygon(E, numpy.ones(4), Z2, I2, BOX)
    assert out['status'] == ref.FULL and abs(out['area'] - 4.0) < 1e-12
    assert numpy.allclose(out['vertices'], [[-1, -1], [1, -1], [1, 1], [-1, 1]])      # ascending atan2 about the mean
    assert [e for e in out['edge_rows']] == [{3}, {0}, {1}, {2}]


def test_reference_triangle_with_a_redundant_row():
    E = numpy.array([[0, -1.0], [1, 1], [-1, 1], [0, 1]])
    out = ref.slice_polygon(E, numpy.array([0, 1, 1, 5.0]), Z2, I2, BOX)
    assert out['status'] == ref.FULL and len(out['vertices']) == 3 and abs(out['area'] - 1.0) < 1e-12
    assert all(3 not in e for e in out['edge_rows'])


def test_reference_hexagon_and_rows_through_a_vertex():
    ang = numpy.arange(6) * numpy.pi / 3
    E = numpy.stack([numpy.cos(ang), numpy.sin(ang)], axis=1)
    v = numpy.array([1.0, 1.0 / numpy.sqrt(3.0)])
    t = numpy.array([numpy.cos(numpy.pi / 6), numpy.sin(numpy.pi / 6)])
    out = ref.slice_polygon(numpy.vstack([E, t]), numpy.concatenate([numpy.ones(6), [t @ v]]), Z2, I2, BOX)
    assert out['status'] == ref.FULL and len(out['vertices']) == 6
    assert abs(out['area'] - 2 * numpy.sqrt(3.0)) < 1e-12
    assert all(6 not in e for e in out['edge_rows'])        # the tangent row touches the vertex only: no edge


def test_reference_segment_empty_and_cut():
    E = numpy.array([[1.0, 0], [-1, 0], [0, 1], [0, -1]])
    assert ref.slice_polygon(E, numpy.array([0.5, -0.5, 1, 1]), Z2, I2, BOX)['status'] == ref.LOWDIM
    assert ref.slice_polygon(E, numpy.array([-1.0, -1, 1, 1]), Z2, I2, BOX)['status'] == ref.EMPTY
    cut = ref.slice_polygon(E[:1], numpy.array([1.0]), Z2, I2, BOX)
    assert cut['status'] == ref.FULL | ref.CUT and abs(cut['area'] - 24.0) < 1e-12
    # a row constant on the plane, violated: empty
    E4 = numpy.vstack([numpy.eye(4), [[0, 0, 1.0, 0]]])
    U = numpy.zeros((4, 2)); U[0, 0] = U[1, 1] = 1
    assert ref.slice_polygon(E4, numpy.array([1, 1, 1, 1, 0.1]), numpy.array([0, 0, 0.5, 0]), U, BOX)['status'] == ref.EMPTY


def test_reference_interval():
    E = numpy.array([[1.0], [-1.0]])
    assert numpy.allclose(ref.slice_interval(E, numpy.array([1.0, 2.0]), [0.0], [1.0], (-5.0, 5.0))[:2], (-2.0, 1.0))


# ---- argument checks, before the device is touched ---------------------------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError('the device was touched')

    def __call__(self, *a, **k):
        raise AssertionError('the device was touched')


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, 'load', _NoDevice())
    monkeypatch.setattr(_lib, 'lp_solve_batch', _NoDevice())


class _Prog:
    def __init__(self, n_t, A_t=None, b_t=None):
        self.n_t = n_t
        self.A_t = numpy.vstack([numpy.eye(n_t), -numpy.eye(n_t)]) if A_t is None else A_t
        self.b_t = numpy.ones((2 * n_t, 1)) if b_t is None else b_t

    def num_t(self):
        return self.n_t


def _solution(n_t, rows=4, **kw):
    from ppopt_amd import CriticalRegion
    E = numpy.vstack([numpy.eye(n_t), -numpy.eye(n_t)])
    E = numpy.vstack([E] * (rows // len(E) + 1))[:rows]
    cr = CriticalRegion(numpy.zeros((1, n_t)), numpy.zeros((1, 1)), numpy.zeros((1, n_t)), numpy.zeros((1, 1)), E, numpy.ones((rows, 1)),
                        [0], [], [])
    return Solution(_Prog(n_t, **kw), [cr])


def test_slice_2d_rejects_bad_arguments(no_device):
    s2 = _solution(2)
    for dims in ((0, 0), (0, 2), (1,), (-1, 0)):
        with pytest.raises(ValueError, match='dims'):
            s2.slice_2d(dims=dims, box=BOX)
    s4 = _solution(4)
    with pytest.raises(ValueError, match='fixed'):
        s4.slice_2d(box=BOX)
    with pytest.raises(ValueError, match='length 4'):
        s4.slice_2d(fixed=numpy.zeros(3), box=BOX)
    with pytest.raises(ValueError, match='fixed'):
        s4.slice_2d(fixed={2: 0.0}, box=BOX)
    with pytest.raises(ValueError, match='plane'):
        s4.slice_2d(plane=(numpy.zeros(4), numpy.zeros((3, 2))), box=BOX)
    with pytest.raises(ValueError, match='box'):
        s2.slice_2d(box=(1.0, 0.0, 0.0, 1.0))
    with pytest.raises(ValueError, match='box'):
        s2.slice_2d(box=(0.0, 0.0, numpy.inf, 1.0))
    # an unbounded parameter set and no box: refused before the four LPs
    half = _solution(2, A_t=numpy.array([[1.0, 0.0], [0.0, 1.0]]), b_t=numpy.ones((2, 1)))
    with pytest.raises(ValueError, match='unbounded'):
        half.slice_2d()
    strip = _solution(3, A_t=numpy.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 0, 1.0], [0, 0, -1.0]]), b_t=numpy.ones((4, 1)))
    with pytest.raises(ValueError, match='unbounded'):
        strip.slice_2d(fixed={2: 0.0})
    with pytest.raises(ValueError, match='unbounded'):
        half.slice_1d(numpy.zeros(2), numpy.array([-1.0, 0.0]))
    # too many rows in a region: MpcError from the library wrapper, still before any launch
    with pytest.raises(_lib.MpcError, match='256 rows'):
        _solution(2, rows=257).slice_2d(box=BOX)


def test_lib_rejects_bad_arguments(no_device):
    ef = numpy.hstack([numpy.ones((4, 1)), numpy.vstack([I2, -I2])])
    off = numpy.array([0, 4])
    for kw, what in ((dict(box=(0, 0, 0, 1)), 'box'), (dict(box=(0, 0, 1)), 'box'), (dict(U=numpy.eye(3)[:, :2]), 'U'),
                     (dict(eps=0.0), 'eps'), (dict(eps=1.5), 'eps')):
        args = dict(row_off=off, ef_rows=ef, theta_0=Z2, U=I2, box=BOX)
        args.update(kw)
        with pytest.raises(_lib.MpcError, match=what):
            _lib.slice_polygons(**args)
    with pytest.raises(_lib.MpcError, match='dimension'):
        _lib.slice_polygons(numpy.array([0, 1]), numpy.ones((1, 66)), numpy.zeros(65), numpy.zeros((65, 2)), BOX)
    with pytest.raises(_lib.MpcError, match='256 rows'):
        _lib.slice_polygons(numpy.array([0, 300]), numpy.ones((300, 3)), Z2, I2, BOX)
    with pytest.raises(_lib.MpcError, match='ef_rows'):
        _lib.slice_polygons(off, ef[:3], Z2, I2, BOX)
    with pytest.raises(_lib.MpcError, match='row_off'):
        _lib.slice_polygons(numpy.array([1, 4]), ef, Z2, I2, BOX)
    with pytest.raises(_lib.MpcError, match='t_range'):
        _lib.slice_intervals(off, ef, Z2, [1.0, 0.0], (1.0, 1.0))
    with pytest.raises(_lib.MpcError, match='same length'):
        _lib.slice_intervals(off, ef, Z2, [1.0, 0.0, 0.0], (0.0, 1.0))
    with pytest.raises(_lib.MpcError, match='dimensions'):
        slice_polytopes([Polytope(I2, numpy.ones(2)), Polytope(numpy.eye(3), numpy.ones(3))], Z2, I2, BOX)


def test_no_cpu_fallback_without_gpu():
    L = _lib.load()
    if L.mpc_device_count() > 0:
        pytest.skip('a GPU is present')
    ef = numpy.hstack([numpy.ones((4, 1)), numpy.vstack([I2, -I2])])
    with pytest.raises(_lib.MpcError):
        _lib.slice_polygons(numpy.array([0, 4]), ef, Z2, I2, BOX)
    with pytest.raises(_lib.MpcError):
        _lib.slice_intervals(numpy.array([0, 4]), ef, Z2, [1.0, 0.0], (-1.0, 1.0))


# ---- drawing, on a synthetic slice --------------------------------------------------------------------------------------
def _synthetic_slice():
    sq = numpy.array([[-1.0, -1], [1, -1], [1, 1], [-1, 1]])
    tri = numpy.array([[1.5, 0.5], [2.5, 0.5], [2.0, 1.5]])
    return SolutionSlice(regions=numpy.arange(4), vertices=[sq, tri, numpy.zeros((0, 2)), numpy.array([[0.0, 2.0], [1.0, 2.0]])],
                         edge_rows=[numpy.arange(4), numpy.arange(3), numpy.zeros(0, int), numpy.arange(2)],
                         areas=numpy.array([4.0, 0.5, 0.0, 0.0]),
                         status=numpy.array([_lib.MPC_SLICE_FULL, _lib.MPC_SLICE_FULL | _lib.MPC_SLICE_CUT, _lib.MPC_SLICE_EMPTY,
                                             _lib.MPC_SLICE_LOWDIM]),
                         theta_0=Z2, U=I2, box=BOX)


def test_plot_slice_draws_one_patch_per_full_polygon():
    import matplotlib
    matplotlib.use('Agg')
    from matplotlib import pyplot
    from ppopt_amd import plot
    sl = _synthetic_slice()
    assert sl.full().tolist() == [True, True, False, False]
    ax = plot.plot_slice(sl, seed=0)
    paths = ax.collections[0].get_paths()
    assert len(paths) == 2
    assert ax.get_xlim() == (-3.0, 3.0)
    pyplot.close(ax.figure)


def test_sort_clockwise_and_vertex_enumeration():
    from ppopt_amd import plot
    rng = numpy.random.default_rng(0)
    sq = [numpy.array(v, dtype=float) for v in ([1, 1], [-1, -1], [1, -1], [-1, 1])]
    out = plot.sort_clockwise([sq[k] for k in rng.permutation(4)])
    assert numpy.allclose(numpy.array(out), [[-1, -1], [1, -1], [1, 1], [-1, 1]])
    # three rows through (1, 1): the vertex once (the reference's LP per pair gives it three times)
    A = numpy.array([[1.0, 0], [0, 1], [1, 1], [-1, 0], [0, -1]])
    b = numpy.array([1.0, 1, 2, 1, 1])
    V = plot.vertex_enumeration_2d(A, b)
    assert len(V) == 4
    assert numpy.allclose(numpy.array(plot.sort_clockwise(V)), [[-1, -1], [1, -1], [1, 1], [-1, 1]])


def test_plotly_plot_names_the_missing_package(monkeypatch):
    import sys
    from ppopt_amd import plot
    for name in ('plotly', 'plotly.graph_objects'):
        monkeypatch.setitem(sys.modules, name, None)          # as if plotly were not installed
    with pytest.raises(ImportError, match='plotly'):
        plot.plotly_plot(_solution(2), show=False)


def test_parametric_plot_refuses_a_solution_that_is_not_2d_without_fixed(capsys, no_device):
    from ppopt_amd import plot
    assert plot.parametric_plot(_solution(3), show=False) is None
    assert 'not 2D' in capsys.readouterr().out
    assert plot.parametric_plot_1D(_solution(2), show=False) is None
    assert 'not 1D' in capsys.readouterr().out
