"""Hit-and-run without a GPU: the CPU reference of the chain (tests/hit_and_run_reference.py) against known answers and the
distribution tests, the host-side helpers of ppopt_amd.geometry, and the input checks that refuse bad sizes before the device is
touched."""
import numpy
import pytest

import hit_and_run_reference as hr
from ppopt_amd import _lib
from ppopt_amd.geometry import Polytope, find_extents, hit_and_run_batch, sample_program_theta_space


@pytest.mark.parametrize('counter, key, want', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    assert tuple(int(v) for v in hr.philox4x32_10(*counter, *key)) == want


def test_u53_extremes():
    assert hr.u53(0, 0) == 0.0
    top = hr.u53(0xffffffff, 0xffffffff)
    assert top == 1.0 - 2.0 ** -53 and top < 1.0
    assert hr.u53(0, 1 << 6) == 2.0 ** -53          # the lowest bit that counts
    assert hr.u53(0x1f, 0x3f) == 0.0                # the discarded bits


def test_reference_chain_stays_inside():
    rng = numpy.random.default_rng(3)
    A = rng.standard_normal((40, 5))
    b = numpy.ones(40)
    X, st = hr.chains(A, b, numpy.zeros(5), 300, 4, 5, seed=9)
    assert (st == 0).all()
    assert numpy.max(X.reshape(-1, 5) @ A.T - b) <= 1e-12


def test_reference_statuses():
    A, b = hr.box(numpy.zeros(3), numpy.ones(3))
    _, st = hr.chains(A, b, numpy.full(3, 2.0), 4, 1, 3, seed=1)
    assert (st == 1).all()
    X, st = hr.chains(numpy.array([[1.0, 0.0]]), numpy.array([1.0]), numpy.zeros(2), 4, 1, 3, seed=1)   # half-plane
    assert (st == 2).all() and numpy.isnan(X).all()


# ---- the distribution tests at a reduced N: the thresholds hold for the reference chain --------------------------------------
N_CPU = 3000
STEPS = 1000      # geometry.DEFAULT_N_STEPS


def test_reference_distribution_unit_box():
    A, b = hr.box(numpy.zeros(8), numpy.ones(8))
    X, _ = hr.chains(A, b, numpy.full(8, 0.5), N_CPU, 1, 100, seed=7)
    ks, mean = hr.check_uniform_box(X[:, 0], 0.0, 1.0)
    assert ks <= 1.0 and mean <= 1.0, (ks, mean)


def test_reference_distribution_simplex():
    A, b = hr.simplex(8)
    X, _ = hr.chains(A, b, numpy.full(8, 1 / (8 + numpy.sqrt(8))), N_CPU, 1, 100, seed=7)
    assert hr.check_simplex(X[:, 0]) <= 1.0


def test_reference_distribution_elongated_box():
    """The 10:1 box in 8 dimensions sets the default step count: 1,000 steps mix it, 300 do not."""
    hi = numpy.r_[10.0, numpy.ones(7)]
    A, b = hr.box(numpy.zeros(8), hi)
    X, _ = hr.chains(A, b, hi / 2, N_CPU, 1, STEPS, seed=7)
    ks, mean = hr.check_uniform_box(X[:, 0], 0.0, hi)
    assert ks <= 1.0 and mean <= 1.0, (ks, mean)
    X, _ = hr.chains(A, b, hi / 2, N_CPU, 1, 300, seed=7)
    assert hr.check_uniform_box(X[:, 0], 0.0, hi)[0] > 1.0      # the test can fail: too few steps are seen


def test_reference_distribution_rotated_box_and_hexagon():
    R = hr.rotation(8, 1)
    A, b = hr.box(numpy.zeros(8), numpy.ones(8))
    X, _ = hr.chains(A @ R.T, b, R @ numpy.full(8, 0.5), N_CPU, 1, 100, seed=5)
    ks, mean = hr.check_uniform_box(X[:, 0] @ R, 0.0, 1.0)
    assert ks <= 1.0 and mean <= 1.0, (ks, mean)
    A, b = hr.hexagon()
    X, _ = hr.chains(A, b, numpy.zeros(2), N_CPU, 1, 100, seed=3)
    stat, limit = hr.chi2_cells(hr.hexagon_cells(X[:, 0]), 12)
    assert stat <= limit, (stat, limit)


# ---- host helpers and input checks of ppopt_amd.geometry ----------------------------------------------------------------------
def test_find_extents():
    A, b = hr.box(-numpy.ones(2), numpy.ones(2))
    assert find_extents(A, b, numpy.array([1.0, 0.0]), numpy.zeros(2)) == 1.0
    assert find_extents(A, b, numpy.array([-1.0, 0.0]), numpy.array([0.5, 0.0])) == 1.5
    d = numpy.array([1.0, 1.0]) / numpy.sqrt(2)
    assert find_extents(A, b, d, numpy.zeros(2)) == pytest.approx(numpy.sqrt(2))
    assert find_extents(numpy.array([[1.0, 0.0]]), numpy.array([1.0]), numpy.array([0.0, 1.0]), numpy.zeros(2)) == float('inf')
    assert find_extents(A, b.reshape(-1, 1), numpy.array([[0.0], [1.0]]), numpy.zeros((2, 1))) == 1.0    # column vectors


class _NoDevice:
    """Fails the test if the device is touched."""
    def __call__(self, *a, **k):
        raise AssertionError('the device was touched')


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, 'load', _NoDevice())
    monkeypatch.setattr(_lib, 'lp_solve_batch', _NoDevice())


def test_batch_rejects_bad_input_before_the_device(no_device):
    A, b = hr.box(numpy.zeros(65), numpy.ones(65))
    with pytest.raises(_lib.MpcError, match='n <= 64'):
        hit_and_run_batch(Polytope(A, b))
    rng = numpy.random.default_rng(0)
    with pytest.raises(_lib.MpcError, match='256 rows'):
        hit_and_run_batch(Polytope(rng.standard_normal((257, 3)), numpy.ones(257)))
    with pytest.raises(_lib.MpcError, match='rows'):
        hit_and_run_batch(Polytope(numpy.eye(3), numpy.ones(4)))
    with pytest.raises(_lib.MpcError, match='dimensions'):
        hit_and_run_batch([Polytope(numpy.eye(3), numpy.ones(3)), Polytope(numpy.eye(2), numpy.ones(2))])
    A, b = hr.box(numpy.zeros(2), numpy.ones(2))
    with pytest.raises(_lib.MpcError, match='starts'):
        hit_and_run_batch([Polytope(A, b)], starts=numpy.zeros((2, 2)))
    with pytest.raises(_lib.MpcError, match='2\\^32'):
        hit_and_run_batch(Polytope(A, b), samples=1 << 16, n_steps=1 << 16)
    with pytest.raises(_lib.MpcError):
        hit_and_run_batch(Polytope(A, b), chains=0)
    with pytest.raises(_lib.MpcError, match='2\\^32'):
        _lib.hit_and_run(numpy.array([0, 4]), numpy.hstack([b[:, None], A]), numpy.zeros((1, 2)), 1, 1 << 20, 1 << 12, 0)
    with pytest.raises(_lib.MpcError, match='row_off'):
        _lib.hit_and_run(numpy.array([0, 300]), numpy.zeros((300, 3)), numpy.zeros((1, 2)), 1, 1, 1, 0)


def test_theta_space_sampling_rejects_bad_input_before_the_device(no_device):
    class Prog:
        A_t = numpy.vstack([numpy.eye(70), -numpy.eye(70)])
        b_t = numpy.ones((140, 1))
    with pytest.raises(_lib.MpcError, match='parameter set'):
        sample_program_theta_space(Prog(), 10)
    Prog.A_t, Prog.b_t = numpy.vstack([numpy.eye(2), -numpy.eye(2)]), numpy.ones((4, 1))
    with pytest.raises(_lib.MpcError):
        sample_program_theta_space(Prog(), 10, n_steps=1 << 32)


def test_no_cpu_fallback_without_gpu():
    L = _lib.load()
    if L.mpc_device_count() > 0:
        pytest.skip('a GPU is present')
    A, b = hr.box(numpy.zeros(2), numpy.ones(2))
    with pytest.raises(_lib.MpcError):
        _lib.hit_and_run(numpy.array([0, 4]), numpy.hstack([b[:, None], A]), numpy.full((1, 2), 0.5), 4, 1, 10, 0)
    with pytest.raises(_lib.MpcError):
        hit_and_run_batch(Polytope(A, b), starts=numpy.full((1, 2), 0.5))
