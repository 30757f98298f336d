"""The exact union check (tests/merge_exact_reference.py) on answers worked out by hand, and the CPU reference merger under that check on
every case of tests/merge_cases.py: no device."""
import numpy
import pytest

import merge_cases
import merge_exact_reference as exact

TOL = 1e-8


def _box(lo, hi):
    n = len(lo)
    return numpy.vstack([numpy.eye(n), -numpy.eye(n)]), numpy.concatenate([numpy.asarray(hi, float), -numpy.asarray(lo, float)])


def test_chebyshev_radius():
    assert exact.chebyshev_radius(*_box((0, 0), (2, 1))) == pytest.approx(0.5, abs=1e-12)
    assert exact.chebyshev_radius(*_box((0, 0, 0), (1, 1, 1))) == pytest.approx(0.5, abs=1e-12)
    # rows that are not unit rows: the triangle x, y >= 0, 3 x + 4 y <= 12 has the inradius (3 + 4 - 5) / 2 = 1
    assert exact.chebyshev_radius([[-2, 0], [0, -5], [3, 4]], [0, 0, 12]) == pytest.approx(1.0, abs=1e-12)
    assert exact.chebyshev_radius([[1.0], [-1.0]], [1.0, -2.0]) == pytest.approx(-0.5, abs=1e-12)      # empty: 2 <= x <= 1
    assert exact.chebyshev_radius([[1.0, 0.0]], [0.0]) == numpy.inf
    assert exact.chebyshev_radius([[0.0, 0.0], [1.0, 0.0]], [-1.0, 0.0]) == -numpy.inf               # 0 <= -1


def test_square_against_its_two_halves():
    sq, left, right = _box((0, 0), (1, 1)), _box((0, 0), (0.5, 1)), _box((0.5, 0), (1, 1))
    assert exact.union_defect(sq, [left, right], TOL) == (0.0, 0.0)
    # one half alone: the other half is outside (radius 1/4), nothing is missing
    out, miss = exact.union_defect(sq, [left], TOL)
    assert out == pytest.approx(0.25, abs=1e-12) and miss == 0.0
    # the order of the others does not matter, and a polytope that only touches is skipped
    far = _box((1, 0), (2, 1))
    assert exact.difference_radius(*sq, [far, right, left], TOL) == 0.0
    assert exact.difference_radius(*sq, [far], TOL) == pytest.approx(0.5, abs=1e-12)


def test_envelope_of_an_ell_against_the_ell():
    ell = [_box((0, 0), (1, 1)), _box((1, 0), (2, 1)), _box((0, 1), (1, 2))]
    out, miss = exact.union_defect(_box((0, 0), (2, 2)), ell, TOL)
    assert out == pytest.approx(0.5, abs=1e-12)     # the missing unit square [1, 2]^2
    assert miss == 0.0
    # the convex hull of the L instead of its box: x + y <= 3 leaves the triangle (1,1), (2,1), (1,2), inradius 1 - 1 / sqrt 2
    E, f = _box((0, 0), (2, 2))
    out, miss = exact.union_defect((numpy.vstack([E, [[1.0, 1.0]]]), numpy.append(f, 3.0)), ell, TOL)
    assert out == pytest.approx(1.0 - numpy.sqrt(0.5), abs=1e-12) and miss == 0.0


@pytest.mark.parametrize('delta', [1e-6, 1e-3, 0.25])
def test_a_row_shifted_inward_misses_half_the_shift(delta):
    left, right = _box((0, 0), (1, 1)), _box((1, 0), (2, 1))
    out, miss = exact.union_defect(_box((0, 0), (2 - delta, 1)), [left, right], TOL)
    assert out == 0.0
    assert miss == pytest.approx(delta / 2, rel=1e-9, abs=1e-14)      # the strip [2 - delta, 2] x [0, 1] of the right member
    # shifted outward instead: delta / 2 outside, nothing missing
    out, miss = exact.union_defect(_box((0, 0), (2 + delta, 1)), [left, right], TOL)
    assert out == pytest.approx(delta / 2, rel=1e-9, abs=1e-14) and miss == 0.0


def test_below_tol_is_nothing():
    left, right = _box((0, 0), (1, 1)), _box((1, 0), (2, 1))
    assert exact.union_defect(_box((0, 0), (2 - 1e-8, 1)), [left, right], TOL) == (0.0, 0.0)     # a strip of radius 5e-9 <= tol


def test_unbounded_half_strips():
    a = (numpy.array([[0.0, 1], [0, -1], [1, 0]]), numpy.array([1.0, 0, 0]))      # 0 <= y <= 1, x <= 0
    b = (numpy.array([[0.0, 1], [0, -1], [-1, 0]]), numpy.array([1.0, 0, 0]))     # 0 <= y <= 1, x >= 0
    strip = (numpy.array([[0.0, 1], [0, -1]]), numpy.array([1.0, 0]))
    assert exact.chebyshev_radius(*a) == pytest.approx(0.5, abs=1e-12)
    assert exact.union_defect(strip, [a, b], TOL) == (0.0, 0.0)
    out, miss = exact.union_defect(strip, [a], TOL)
    assert out == pytest.approx(0.5, abs=1e-12) and miss == 0.0
    # the strip 0 <= y <= 2 instead: the unbounded strip 1 <= y <= 2 is outside
    out, miss = exact.union_defect((strip[0], numpy.array([2.0, 0])), [a, b], TOL)
    assert out == pytest.approx(0.5, abs=1e-12) and miss == 0.0
    # a half-plane against the half-strips: what is outside holds balls of any radius
    assert exact.union_defect((numpy.array([[0.0, -1]]), numpy.array([0.0])), [a, b], TOL) == (numpy.inf, 0.0)


def test_intervals():
    iv = lambda lo, hi: (numpy.array([[1.0], [-1.0]]), numpy.array([hi, -lo]))
    assert exact.union_defect(iv(0, 3), [iv(0, 1), iv(1, 2), iv(2, 3)], TOL) == (0.0, 0.0)
    out, miss = exact.union_defect(iv(0, 3), [iv(0, 1), iv(2, 3)], TOL)
    assert out == pytest.approx(0.5, abs=1e-12) and miss == 0.0
    out, miss = exact.union_defect(iv(0.5, 3), [iv(0, 1), iv(1, 3.5)], TOL)
    assert out == 0.0 and miss == pytest.approx(0.25, abs=1e-12)      # [0, 0.5] and [3, 3.5], both of radius 1/4


@pytest.mark.parametrize('name', sorted(merge_cases.CASES))
def test_reference_forms_true_unions_on_the_generated_cases(name):
    """The rules themselves give true unions on every committed case, the reference meets no knife-edge LP value (so the device tests
    of tests/test_gpu_merge_exact.py need no exemption) and merges at least once."""
    src = merge_cases.build(name)
    want, info = merge_cases.reference(name)
    assert info['knife'] == 0
    assert len(want) < len(src) and info['rounds'] >= 1
    assert sorted(i for r in want.critical_regions for i in r.members) == list(range(len(src)))
    for r in want.critical_regions:
        if len(r.members) > 1:
            out, miss = exact.union_defect(merge_cases.rows_of(r), [merge_cases.rows_of(src.critical_regions[i]) for i in r.members], TOL)
            print(name, r.members, out, miss)
            assert out <= 10 * TOL and miss <= 10 * TOL, (r.members, out, miss)


def test_the_generated_cases_reach_what_they_are_for():
    par = merge_cases.CASES
    assert {p['n'] for p in par.values()} >= {2, 3, 4, 8, 16}
    assert {p['cuts'] for p in par.values()} >= {3, 4, 5, 6}
    assert {p.get('nlaws', 1) for p in par.values()} == {1, 2, 3}
    assert any(p.get('drop') for p in par.values()) and any(p.get('grown') for p in par.values())
    assert any(p.get('thin', 1e-3) < 1e-6 for p in par.values())
    # the padded case tests pairs with a side of more than 64 and of more than 128 rows
    name = next(k for k, p in par.items() if p.get('pad'))
    sides = [max(len(p), len(q)) for p, q, _, _, _ in merge_cases.reference(name)[1]['tested']]
    assert any(64 < s <= 128 for s in sides) and any(s > 128 for s in sides)
    # thin cells exist where they are asked for (a sliver between two parallel cuts)
    name = next(k for k, p in par.items() if p.get('sliver'))
    radii = [exact.chebyshev_radius(*merge_cases.rows_of(r)) for r in merge_cases.build(name).critical_regions]
    assert min(radii) < 1e-5
    # the rounds and groups the cases are meant to reach
    infos = [merge_cases.reference(k)[1] for k in par]
    assert max(i['rounds'] for i in infos) >= 3 and max(i['groups'] for i in infos) >= 3
