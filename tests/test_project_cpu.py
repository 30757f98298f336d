"""Projections of polytopes without a device: the CPU reference on cases whose answers are derived by hand
(tests/project_cases.py), the host layer over a stand-in for _lib.project_rows built on the reference, and every refusal that comes
before a launch."""
import numpy
import pytest

import exit_cases as ec
import project_cases as pc
import project_reference as pr
import reduce_cases as rc
from ppopt_amd import _lib
from ppopt_amd.geometry import (Polytope, ProjectedRows, affine_image, controllable_pre, minkowski_sum, project_polytopes, project_rows_of)
from ppopt_amd.geometry import project as pj

TOL = pc.TOL
HAND = pc.hand_cases()


# ---- the reference on the hand cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,rows,n_elim,status,want,peak', HAND, ids=[c[0] for c in HAND])
def test_reference_on_the_hand_cases(name, rows, n_elim, status, want, peak):
    r = pr.project_one(rows, n_elim, TOL)
    assert r.status == status and r.peak == peak and not r.knife
    if want is None:
        assert len(r.rows) == 0
    else:
        assert r.rows.shape == want.shape and numpy.max(numpy.abs(r.rows - want)) <= 1e-12
    if name in ('square', 'strip'):
        assert r.wide == 2                     # both ends of an interval: the set beyond either is a ray


def test_reference_steps_alone():
    """the zero combination that empties a set, which the thin test hides from project_one; Z alone; the row limit"""
    empty = [c for c in HAND if c[0] == 'empty'][0][1]
    new, total, is_empty, nu = pr.eliminate(empty, TOL)
    assert is_empty and total == 1 and len(new) == 0 and nu == numpy.inf
    new, total, is_empty, nu = pr.eliminate(numpy.array([[1.0, 1.0, 0.0], [0.0, -1.0, 0.0]]), TOL)
    assert not is_empty and total == 2 and new.tolist() == [[1.0, 1.0], [0.0, -1.0]]
    assert pr.eliminate(pc.opposing(24), TOL)[1] == 576
    # a coefficient below the class threshold that is not zero: the row is Z and is scaled again
    new, total, _, _ = pr.eliminate(numpy.array([[1.0, 1.0, 1e-13], [0.0, -1.0, 0.0]]), TOL)
    assert total == 2 and new.tolist() == [[1.0, 1.0], [0.0, -1.0]]


def test_reference_without_elimination_gives_the_masks_of_the_reduce_cases():
    for name, rows, kept, thin in rc.hand_cases():
        r = pr.project_one(rows, 0, TOL)
        if thin:
            assert r.status == pr.THIN and len(r.rows) == 0
        else:
            assert r.status == pr.OK and r.rows.tobytes() == rows[numpy.asarray(kept, dtype=bool)].tobytes(), name


@pytest.mark.parametrize('case', pc.SETS[:3], ids=pc.IDS[:3])
def test_the_small_seeds_have_no_knife_polytope_and_no_small_combination(case):
    n, n_elim, tangent, k, seed = case
    polys = pc.seeded_set(*case)
    res = pr.project_reference(polys, n_elim, TOL)
    assert len(polys) == k and all(len(p) == 2 * n + tangent for p in polys)
    assert not any(r.knife for r in res) and all(r.status == pr.OK for r in res)
    assert min(r.nu for r in res) >= 1e-4
    assert all(abs(v - TOL) > pr.KNIFE for r in res for v in r.lp)
    if n - n_elim > 1:
        assert not any(r.wide for r in res)    # unbounded runs only in projections onto a line


# ---- the host layer over a stand-in for the device ---------------------------------------------------------------------------------------
def _stand_in(monkeypatch, calls=None):
    """_lib.project_rows answered by the reference, in the terms of the binding"""
    def project_rows(off, ef, n_elim, start, tol, out_cap=512, device=0):
        off, ef = numpy.asarray(off), numpy.asarray(ef)
        n = len(off) - 1
        res = [pr.project_one(ef[off[q]:off[q + 1]], n_elim, tol, out_cap) for q in range(n)]
        if calls is not None:
            calls.append((n, n_elim, ef.copy(), None if start is None else numpy.array(start, copy=True)))
        k = ef.shape[1] - 1 - n_elim
        out_off = numpy.concatenate([[0], numpy.cumsum([len(r.rows) for r in res])]).astype(numpy.int64)
        stats = {key: 0 for key in ('thin', 'whole', 'too_large', 'steps', 'rows_made', 'pivots')}
        stats.update(polytopes=n, lps=sum(len(r.lp) for r in res), wide=sum(r.wide for r in res), ms=0.0)
        return (out_off, numpy.vstack([r.rows.reshape(-1, k + 1) for r in res]), numpy.array([r.status for r in res], dtype=numpy.int32),
                numpy.array([r.wide for r in res], dtype=numpy.int32), numpy.array([r.peak for r in res], dtype=numpy.int32), numpy.zeros((n, k)), stats)
    monkeypatch.setattr(_lib, 'project_rows', project_rows)


def _same_set(rows_a, rows_b, tol=1e-9):
    """two bounded polytopes of rows [o | n] are equal: every row of one has the other's support value in its direction"""
    for mine, other in ((rows_a, rows_b), (rows_b, rows_a)):
        for row in mine:
            s = numpy.linalg.norm(row[1:])
            if abs(pr.support(other, row[1:] / s) - row[0] / s) > tol * (1 + abs(row[0] / s)):
                return False
    return True


def test_project_rows_of_permutes_keep_and_order_and_leaves_the_source(monkeypatch):
    calls = []
    _stand_in(monkeypatch, calls)
    tri = [c for c in HAND if c[0] == 'triangle_x'][0][1]
    simplex = [c for c in HAND if c[0] == 'simplex'][0][1]
    off, ef = ec.csr([tri])
    before = (off.copy(), ef.copy())
    onto_x = project_rows_of(off, ef, 2, [0], tol=TOL)
    onto_y = project_rows_of(off, ef, 2, [1], tol=TOL, start=numpy.array([[1.0, 0.25]]))
    assert isinstance(onto_x, ProjectedRows) and len(onto_x) == 1
    assert off.tobytes() == before[0].tobytes() and ef.tobytes() == before[1].tobytes()
    assert numpy.allclose(onto_x.rows, [[2.0, 1.0], [0.0, -1.0]], atol=1e-12) and onto_x.row_off.tolist() == [0, 2]
    assert numpy.allclose(onto_y.rows, [[0.0, -1.0], [1.0, 1.0]], atol=1e-12)
    assert calls[1][2].tobytes() == ef[:, [0, 2, 1]].tobytes() and calls[1][3].tolist() == [[0.25, 1.0]]   # (y, x): x trails
    assert onto_x.stats['rows_before'] == 3 and onto_x.stats['rows_after'] == 2 and onto_x.peak.tolist() == [2]
    # keep in another order: the rows come in the order of keep
    off3, ef3 = ec.csr([simplex])
    xy = project_rows_of(off3, ef3, 3, [0, 1], tol=TOL)
    yx = project_rows_of(off3, ef3, 3, [1, 0], tol=TOL)
    assert xy.rows.shape == (3, 3) and _same_set(xy.rows, yx.rows[:, [0, 2, 1]])
    assert calls[-1][2].tobytes() == ef3[:, [0, 2, 1, 3]].tobytes()
    # the elimination order: the first coordinate of ``order`` is the last column
    project_rows_of(off3, ef3, 3, [1], tol=TOL)
    assert calls[-1][2].tobytes() == ef3[:, [0, 2, 1, 3]].tobytes()          # default: descending index, 2 goes first
    line = project_rows_of(off3, ef3, 3, [1], tol=TOL, order=[0, 2])
    assert calls[-1][2].tobytes() == ef3[:, [0, 2, 3, 1]].tobytes() and calls[-1][1] == 2
    assert _same_set(line.rows, numpy.array([[1.0, 1.0], [0.0, -1.0]]))


def test_polytope_project_and_project_polytopes(monkeypatch):
    _stand_in(monkeypatch)
    tri = Polytope(numpy.array([[0.0, -3.0], [2.0, 2.0], [-1.0, 1.0]]), numpy.array([[0.0], [4.0], [0.0]]))    # not scaled
    A0, b0 = tri.A.copy(), tri.b.copy()
    p = tri.project([0], tol=TOL)
    assert isinstance(p, Polytope) and numpy.allclose(p.rows(), [[2.0, 1.0], [0.0, -1.0]], atol=1e-12)
    assert tri.A.tobytes() == A0.tobytes() and tri.b.tobytes() == b0.tobytes()
    both = project_polytopes([tri, tri], [1], tol=TOL)
    assert len(both) == 2 and both.row_off.tolist() == [0, 2, 4] and [q.A.shape for q in both.polytopes()] == [(2, 1), (2, 1)]
    whole = Polytope(numpy.array([[1.0, 1.0]]), numpy.array([[1.0]])).project([0], tol=TOL)
    assert whole.A.shape == (0, 1) and whole.b.shape == (0, 1)
    with pytest.raises(ValueError, match=r'Polytope.project: the projection is THIN \(peak = 0 rows\)'):
        Polytope(numpy.array([[1.0, 0], [-1.0, 0], [0, 1.0], [0, -1.0]]), numpy.array([[0.0], [0.0], [1.0], [0.0]])).project([0], tol=TOL)
    big = pc.opposing(24)
    with pytest.raises(ValueError, match=r'Polytope.project: the projection is TOO_LARGE \(peak = 576 rows\)'):
        Polytope(big[:, 1:], big[:, :1]).project([0], tol=TOL)


def test_affine_image(monkeypatch):
    calls = []
    _stand_in(monkeypatch, calls)
    sq = ec.box_rows([0, 0], [1, 1])
    P = Polytope(sq[:, 1:].copy(), sq[:, :1].copy())
    # wide M: the sum x + y of the unit square is [0, 2], shifted by 3
    img = affine_image(P, numpy.array([[1.0, 1.0]]), v=[3.0], tol=TOL)
    assert len(calls) == 1 and _same_set(img.rows(), numpy.array([[5.0, 1.0], [-3.0, -1.0]]))
    # invertible M: no call; the image of the square under a shear, by its vertices
    M = numpy.array([[1.0, 0.5], [0.0, 2.0]])
    img = affine_image(P, M, v=[1.0, -1.0], tol=TOL)
    assert len(calls) == 1
    corners = numpy.array([[0.0, 0], [1, 0], [0, 1], [1, 1]]) @ M.T + numpy.array([1.0, -1.0])
    slack = img.b.reshape(1, -1) - corners @ img.A.T
    assert slack.min() >= -1e-12 and numpy.all(numpy.sum(numpy.abs(slack) <= 1e-12, axis=0) == 2)   # every side through two corners
    assert P.A.tobytes() == sq[:, 1:].tobytes()
    with pytest.raises(ValueError, match='affine_image: M has rank below 2: the image is flat'):
        affine_image(P, numpy.array([[1.0, 1.0], [2.0, 2.0]]))
    with pytest.raises(ValueError, match='affine_image: M must be a finite'):
        affine_image(P, numpy.ones((3, 2)))
    with pytest.raises(ValueError, match='affine_image: M must be a finite'):
        affine_image(P, numpy.array([[numpy.nan, 1.0]]))
    with pytest.raises(ValueError, match='affine_image: v must be a finite vector of 1'):
        affine_image(P, numpy.array([[1.0, 1.0]]), v=[1.0, 2.0])
    assert len(calls) == 1


def test_minkowski_sum_of_the_square_and_the_diamond_is_the_octagon(monkeypatch):
    _stand_in(monkeypatch)
    sq = ec.box_rows([0, 0], [1, 1])
    dm = numpy.array([[1.0, sx, sy] for sx in (1.0, -1.0) for sy in (1.0, -1.0)])
    got = minkowski_sum(Polytope(sq[:, 1:], sq[:, :1]), Polytope(dm[:, 1:], dm[:, :1]), tol=TOL)
    assert got.A.shape == (8, 2) and _same_set(got.rows(), pc.octagon())
    with pytest.raises(ValueError, match='minkowski_sum: the polytopes have different dimensions'):
        minkowski_sum(Polytope(sq[:, 1:], sq[:, :1]), Polytope(numpy.ones((1, 3)), numpy.ones((1, 1))))
    nine = ec.box_rows(numpy.zeros(9), numpy.ones(9))
    with pytest.raises(ValueError, match='minkowski_sum: 2 n = 18 > 16'):
        minkowski_sum(Polytope(nine[:, 1:], nine[:, :1]), Polytope(nine[:, 1:], nine[:, :1]))


def test_controllable_pre_of_the_integrator(monkeypatch):
    """x+ = x + u, |u| <= 1, C = [-1, 1]: Pre = [-2, 2]; within [0, 5]: [0, 2]; every target in one call"""
    calls = []
    _stand_in(monkeypatch, calls)
    iv = lambda lo, hi: Polytope(numpy.array([[1.0], [-1.0]]), numpy.array([[float(hi)], [-float(lo)]]))
    got = controllable_pre([iv(-1, 1), iv(3, 4)], [[1.0]], [1.0], iv(-1, 1), tol=TOL)
    assert len(calls) == 1 and calls[0][0] == 2 and calls[0][1] == 1 and got.status.tolist() == [pj.OK, pj.OK]
    assert _same_set(got.rows_of(0), numpy.array([[2.0, 1.0], [2.0, -1.0]])) and _same_set(got.rows_of(1), numpy.array([[5.0, 1.0], [-2.0, -1.0]]))
    cut = controllable_pre(iv(-1, 1), [[1.0]], [[1.0]], iv(-1, 1), within=iv(0, 5), tol=TOL)
    assert _same_set(cut.rows_of(0), numpy.array([[2.0, 1.0], [0.0, -1.0]]))
    none = controllable_pre(iv(-1, 1), [[1.0]], [[1.0]], iv(-1, 1), within=iv(4, 5), tol=TOL)
    assert none.status.tolist() == [pj.THIN] and len(none.rows) == 0
    for bad, text in ((dict(A=[[1.0, 0.0]]), 'A must be a finite square matrix'), (dict(B=[[1.0], [2.0]]), r'B must be a finite \[1, n_u\] matrix'),
                      (dict(U=Polytope(numpy.eye(2), numpy.ones((2, 1)))), 'U has 2 coordinates, B has 1 columns'),
                      (dict(within=Polytope(numpy.eye(2), numpy.ones((2, 1)))), 'within has 2 coordinates, A has 1'),
                      (dict(targets=[]), 'no targets'), (dict(targets=Polytope(numpy.eye(2), numpy.ones((2, 1)))), 'a target has 2 coordinates, A has 1')):
        a = dict(targets=iv(-1, 1), A=[[1.0]], B=[[1.0]], U=iv(-1, 1), within=None)
        a.update(bad)
        with pytest.raises(ValueError, match='controllable_pre: ' + text):
            controllable_pre(a['targets'], a['A'], a['B'], a['U'], within=a['within'])
    with pytest.raises(ValueError, match=r'controllable_pre: n_theta \+ n_u = 17 > 16'):
        box = ec.box_rows(numpy.zeros(9), numpy.ones(9))
        controllable_pre(Polytope(box[:, 1:], box[:, :1]), numpy.eye(9), numpy.ones((9, 8)), Polytope(numpy.eye(8), numpy.ones((8, 1))))
    assert len(calls) == 3


# ---- every refusal comes before the library is loaded ------------------------------------------------------------------------------------
def test_every_argument_error_is_a_value_error_before_the_library_is_loaded(monkeypatch):
    for name in ('project_rows', 'reduce_rows', 'load'):
        monkeypatch.setattr(_lib, name, lambda *a, **k: pytest.fail('the library was reached'))
    sq = ec.box_rows([0, 0], [1, 1])
    good = dict(off=[0, 4], ef=sq, n=2, keep=[0], tol=1e-8, start=None, order=None, out_cap=512)
    nan_row, long_row = sq.copy(), sq.copy()
    nan_row[1, 0] = numpy.nan
    long_row[2, 1] = -2.0
    cases = [(dict(n=0), 'n_theta = 0 is outside 1..16'), (dict(n=17, ef=numpy.zeros((4, 18))), 'n_theta = 17 is outside 1..16'),
             (dict(tol=-1.0), 'tol must be finite'), (dict(tol=numpy.nan), 'tol must be finite'), (dict(tol=numpy.inf), 'tol must be finite'),
             (dict(ef=sq[:, :2]), 'ef_rows must be'), (dict(off=[1, 4]), 'row_off'), (dict(off=[0, 0, 4]), r'every polytope needs 1\.\.512 rows'),
             (dict(off=[0, 513], ef=numpy.tile(sq, (129, 1))[:513]), r'every polytope needs 1\.\.512 rows'),
             (dict(ef=nan_row), 'rows must be finite'), (dict(ef=long_row), 'rows must have unit normals'),
             (dict(start=numpy.array([[numpy.nan, 0.0]])), 'start must be a finite'), (dict(start=numpy.zeros((2, 2))), 'start must be a finite'),
             (dict(keep=[]), 'keep must name at least one coordinate'), (dict(keep=[0, 0]), 'keep must name'), (dict(keep=[2]), 'keep must name'),
             (dict(keep=[-1]), 'keep must name'), (dict(keep=[0.5]), 'keep must name'), (dict(keep=5), 'keep must be a list of coordinates'),
             (dict(order=[0]), r'order must name the eliminated coordinates \[1\]'), (dict(order=[1, 1]), 'order must name'),
             (dict(order=7), 'order must be a list'), (dict(out_cap=0), 'out_cap = 0 is outside 1..512'), (dict(out_cap=513), 'out_cap = 513 is outside'),
             (dict(out_cap=2.5), 'out_cap = 2.5 is outside')]
    for change, text in cases:
        a = dict(good)
        a.update(change)
        with pytest.raises(ValueError, match='project_rows_of: .*' + text):
            project_rows_of(a['off'], a['ef'], a['n'], a['keep'], tol=a['tol'], start=a['start'], order=a['order'], out_cap=a['out_cap'])
    with pytest.raises(ValueError, match='project_polytopes: no polytopes'):
        project_polytopes([], [0])
    with pytest.raises(ValueError, match='project_polytopes: a polytope has no rows, or a row without a normal'):
        project_polytopes(Polytope(numpy.array([[1.0, 0.0], [0.0, 0.0]]), numpy.ones((2, 1))), [0])
    with pytest.raises(ValueError, match='project_polytopes: the polytopes have different dimensions'):
        project_polytopes([Polytope(sq[:, 1:], sq[:, :1]), Polytope(numpy.ones((1, 3)), numpy.ones((1, 1)))], [0])
    with pytest.raises(ValueError, match='Polytope.project: a polytope has no rows, or a row without a normal'):
        Polytope(numpy.zeros((1, 2)), numpy.ones((1, 1))).project([0])
    with pytest.raises(ValueError, match='Polytope.project: keep must name'):
        Polytope(sq[:, 1:], sq[:, :1]).project([0, 1, 2])


def test_the_symbol_is_part_of_the_abi():
    assert 'mpc_project_rows' in _lib.EXPORTED_SYMBOLS
    assert (_lib.PROJECT_OK, _lib.PROJECT_THIN, _lib.PROJECT_WHOLE, _lib.PROJECT_TOO_LARGE) == (pj.OK, pj.THIN, pj.WHOLE, pj.TOO_LARGE) == (0, 1, 2, 3)
