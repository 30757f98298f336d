"""2-D and 1-D slices on the MI355X (mpc_slice_polygons / k_slice_polygons, mpc_slice_intervals / k_slice_intervals) against the
independent scipy reference (tests/slice_reference.py): random polytopes with the hard cases, determinism, solved programs checked
against point location on a grid, and the plots end to end."""
import warnings

import numpy
import pytest

import slice_reference as ref
from ppopt_amd import _lib
from ppopt_amd.geometry import Polytope, slice_polytopes

pytestmark = pytest.mark.gpu


def _polygon(rng, m, centre=(0.0, 0.0), scale=1.0):
    """m rows a_i z <= a_i c + r_i with unit normals at random angles (a bounded polygon once the normals surround the origin)."""
    phi = rng.uniform(-numpy.pi, numpy.pi, m)
    phi[:3] = [0.1, 2.2, -2.0]          # normals that surround the origin
    A = numpy.stack([numpy.cos(phi), numpy.sin(phi)], axis=1) * rng.uniform(0.5, 2.0, (m, 1))
    r = rng.uniform(0.5, 1.0, m) * scale * numpy.linalg.norm(A, axis=1)
    return A, A @ numpy.asarray(centre) + r


def _box_about(centre, half):
    c = numpy.asarray(centre, dtype=float)
    return numpy.array([c[0] - half, c[1] - half, c[0] + half, c[1] + half])


def _hexagon_with_vertex_rows():
    """A regular hexagon, plus at one vertex: a row tangent there (touches only the vertex), and an exact duplicate and a scaled
    copy of an edge row."""
    ang = numpy.arange(6) * numpy.pi / 3
    A = numpy.stack([numpy.cos(ang), numpy.sin(ang)], axis=1)
    b = numpy.ones(6)
    v = numpy.array([1.0, 1.0 / numpy.sqrt(3.0)])          # the vertex between rows 0 and 1
    t = numpy.array([numpy.cos(numpy.pi / 6), numpy.sin(numpy.pi / 6)])
    A = numpy.vstack([A, t, 0.5 * t, A[2], 3.0 * A[4]])
    b = numpy.concatenate([b, [t @ v, 0.5 * t @ v, 1.0, 3.0]])
    return A, b


def planar_cases():
    """(name, E, f, theta_0, U, box) with n_theta = 2, U = I."""
    rng = numpy.random.default_rng(5)
    I2, z2 = numpy.eye(2), numpy.zeros(2)
    out = []
    for m in (3, 4, 8, 17, 64, 200, 256):
        A, b = _polygon(rng, m)
        out.append((f'random_m{m}', A, b, z2, I2, _box_about((0, 0), 3.0)))
    A, b = _polygon(rng, 12)
    dup = numpy.vstack([A, A[3:6], 2.0 * A[7:9], A[0]])
    out.append(('duplicates_and_parallels', dup, numpy.concatenate([b, b[3:6], 2.0 * b[7:9], [b[0] + 0.5]]), z2, I2, _box_about((0, 0), 3.0)))
    A, b = _hexagon_with_vertex_rows()
    out.append(('vertex_rows', A, b, z2, I2, _box_about((0, 0), 2.0)))
    A, b = _polygon(rng, 10, centre=(0.3e-6, -0.2e-6), scale=1e-6)
    out.append(('tiny', A, b, z2, I2, _box_about((0.3e-6, -0.2e-6), 3e-6)))
    A, b = _polygon(rng, 10, centre=(1e6, -2e6), scale=1.0)
    out.append(('far', A, b, z2, I2, _box_about((1e6, -2e6), 3.0)))
    out.append(('wedge_cut_by_box', numpy.array([[1.0, 1.0], [-1.0, 2.0]]), numpy.array([1.0, 0.5]), z2, I2, _box_about((0, 0), 2.0)))
    out.append(('half_plane', numpy.array([[0.3, 1.0]]), numpy.array([0.2]), z2, I2, _box_about((0, 0), 1.0)))
    out.append(('empty', numpy.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0]]), numpy.array([-1.0, -1.0, 1.0]), z2, I2, _box_about((0, 0), 3.0)))
    out.append(('segment', numpy.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]]), numpy.array([0.5, -0.5, 1.0, 1.0]), z2, I2,
                _box_about((0, 0), 3.0)))
    out.append(('point', numpy.array([[1.0, 0.0], [-1.0, 1.0], [-1.0, -1.0]]), numpy.array([0.0, 0.0, 0.0]), z2, I2, _box_about((0, 0), 3.0)))
    out.append(('outside_box', numpy.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]]), numpy.array([11.0, -10.0, 1.0, 1.0]), z2, I2,
                _box_about((0, 0), 3.0)))
    return out


def plane_cases():
    """(name, E, f, theta_0, U, box) in n_theta = 3 .. 64: a box polytope with random rows, cut by a random plane through a point
    inside; plus rows constant on the plane (satisfied, and violated: an empty slice)."""
    rng = numpy.random.default_rng(11)
    out = []
    for n, m in ((3, 10), (4, 40), (8, 64), (16, 100), (33, 200), (64, 256)):
        k = m - 2 * n
        E = numpy.vstack([numpy.eye(n), -numpy.eye(n), rng.standard_normal((k, n))])
        f = numpy.concatenate([rng.uniform(0.5, 2.0, 2 * n), rng.uniform(0.5, 1.5, k) * numpy.linalg.norm(E[2 * n:], axis=1)])
        Q, _ = numpy.linalg.qr(rng.standard_normal((n, 2)))
        theta_0 = rng.uniform(-0.2, 0.2, n)
        out.append((f'plane_n{n}_m{m}', E, f, theta_0, Q, _box_about((0, 0), 2.5)))
    n = 4
    E = numpy.vstack([numpy.eye(n), -numpy.eye(n), [[0, 0, 1.0, 1.0]]])
    U = numpy.zeros((n, 2)); U[0, 0] = U[1, 1] = 1.0
    out.append(('constant_row_satisfied', E, numpy.concatenate([numpy.ones(8), [0.5]]), numpy.array([0, 0, 0.1, 0.2]), U, _box_about((0, 0), 2.0)))
    out.append(('constant_row_violated', E, numpy.concatenate([numpy.ones(8), [0.5]]), numpy.array([0, 0, 0.4, 0.2]), U, _box_about((0, 0), 2.0)))
    return out


ALL = planar_cases() + plane_cases()


def _check(name, E, f, theta_0, U, box, got, k=0):
    vert, edge, count, area, status = got
    want = ref.slice_polygon(E, f, theta_0, U, box)
    assert status[k] == want['status'], (name, int(status[k]), want['status'])
    if (want['status'] & ~ref.CUT) != ref.FULL:
        return
    D = numpy.hypot(box[2] - box[0], box[3] - box[1])
    tol = 1e-9 * (D + 1e-6 * numpy.max(numpy.abs(box)))
    s = int(numpy.concatenate([[0], numpy.cumsum([len(f)])])[k]) + 4 * k
    V = vert[s:s + count[k]]
    assert count[k] == len(want['vertices']), (name, int(count[k]), len(want['vertices']))
    assert numpy.max(numpy.abs(V - want['vertices'])) <= tol, (name, numpy.max(numpy.abs(V - want['vertices'])), tol)
    assert abs(area[k] - want['area']) <= 1e-9 * want['area'] + 1e-12 * D * D, (name, area[k], want['area'])
    for q in range(count[k]):
        assert int(edge[s + q]) in want['edge_rows'][q], (name, q, int(edge[s + q]), want['edge_rows'][q])


@pytest.mark.parametrize('case', ALL, ids=[c[0] for c in ALL])
def test_one_region_against_the_reference(case):
    name, E, f, theta_0, U, box = case
    ef = numpy.hstack([numpy.asarray(f).reshape(-1, 1), E])
    got = _lib.slice_polygons(numpy.array([0, len(f)]), ef, theta_0, U, box)
    _check(name, E, f, theta_0, U, box, got)


def test_batch_equals_single_launches_and_repeats_bit_for_bit():
    """All planar cases in one launch (each with the same plane and box, so the cases' own boxes are replaced by one), against the
    launches of one region each and against a repeat."""
    cases = [c for c in planar_cases() if c[0].startswith(('random', 'dup', 'vertex', 'wedge', 'half', 'empty', 'segment', 'point'))]
    box = _box_about((0, 0), 3.0)
    polys = [Polytope(E, f) for _, E, f, *_ in cases]
    a = slice_polytopes(polys, numpy.zeros(2), numpy.eye(2), box)
    b = slice_polytopes(polys, numpy.zeros(2), numpy.eye(2), box)
    for k, p in enumerate(polys):
        one = slice_polytopes([p], numpy.zeros(2), numpy.eye(2), box)
        for s in (b, one):
            j = 0 if s is one else k
            assert numpy.array_equal(a.vertices[k], s.vertices[j]) and numpy.array_equal(a.edge_rows[k], s.edge_rows[j])
            assert a.areas[k] == s.areas[j] and a.status[k] == s.status[j]
    # the batch against the reference, region by region
    row_off = numpy.concatenate([[0], numpy.cumsum([len(c[2]) for c in cases])])
    ef = numpy.vstack([numpy.hstack([numpy.asarray(f).reshape(-1, 1), E]) for _, E, f, *_ in cases])
    got = _lib.slice_polygons(row_off, ef, numpy.zeros(2), numpy.eye(2), box)
    for k, (name, E, f, *_rest) in enumerate(cases):
        vert, edge, count, area, status = got
        s = int(row_off[k]) + 4 * k
        one = (vert[s:], edge[s:], count[k:k + 1], area[k:k + 1], status[k:k + 1])
        _check(name, E, f, numpy.zeros(2), numpy.eye(2), box, (one[0], one[1], one[2], one[3], one[4]), 0)


def test_intervals_against_a_numpy_clip():
    rng = numpy.random.default_rng(3)
    for n, m in ((1, 2), (2, 9), (5, 40), (64, 256)):
        E = numpy.vstack([numpy.eye(n), -numpy.eye(n), rng.standard_normal((m - 2 * n, n))]) if m >= 2 * n else rng.standard_normal((m, n))
        theta_0 = rng.uniform(-0.1, 0.1, n)
        f = E @ theta_0 + rng.uniform(0.2, 1.0, len(E)) * numpy.linalg.norm(E, axis=1)     # theta_0 inside
        u = rng.standard_normal(n)
        iv, st = _lib.slice_intervals(numpy.array([0, len(f)]), numpy.hstack([f[:, None], E]), theta_0, u, (-5.0, 5.0))
        a, b = E @ u, f - E @ theta_0
        lo, hi = max([-5.0] + list(b[a < 0] / a[a < 0])), min([5.0] + list(b[a > 0] / a[a > 0]))
        assert (st[0] & ~ref.CUT) == ref.FULL and abs(iv[0, 0] - lo) <= 1e-12 * 10 and abs(iv[0, 1] - hi) <= 1e-12 * 10, (n, iv, lo, hi)
        ta, tb, s2 = ref.slice_interval(E, f, theta_0, u, (-5.0, 5.0))
        assert st[0] == s2 and abs(ta - lo) < 1e-9 and abs(tb - hi) < 1e-9
    # empty, a point, cut by the range, and a row constant on the line
    E = numpy.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0]])
    for f, st_want in (([-1.0, -1.0, 1.0], ref.EMPTY), ([0.0, 0.0, 1.0], ref.LOWDIM), ([9.0, 9.0, 1.0], ref.FULL | ref.CUT), ([1.0, 1.0, -1.0], ref.EMPTY)):
        iv, st = _lib.slice_intervals(numpy.array([0, 3]), numpy.hstack([numpy.array(f)[:, None], E]), numpy.zeros(2), [1.0, 0.0], (-2.0, 2.0))
        assert st[0] == st_want, (f, st, st_want)


# ---- solved programs: every region's polygon against the reference, and the polygons against point location on a grid -----------
def _solve(name):
    from ppopt_amd import MPLP_Program, MPQP_Program, problem_generator as pg
    from ppopt_amd.mp_solvers.solve_mpqp import mpqp_algorithm, solve_mpqp
    import bench
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if name == 'c1':
            d = pg.transport_mplp_data()
            prog = MPLP_Program(d['A'], d['b'], d['c'], d['H'], d['A_t'], d['b_t'], d['F'], equality_indices=list(d['equality_indices']))
            return solve_mpqp(prog, mpqp_algorithm.combinatorial)
        if name == 'c2':
            return solve_mpqp(bench.build_program('c2'), mpqp_algorithm.combinatorial)
        if name == 'c3':
            return solve_mpqp(bench.build_program('c3'), mpqp_algorithm.geometric)
        if name == 'rand_4_2_10':
            return solve_mpqp(pg.generate_mpqp(4, 2, 10, 7), mpqp_algorithm.combinatorial)
        if name == 'rand_5_3_8_s3':
            d = pg.generate_mpqp_data(5, 3, 8, 3)
            prog = MPQP_Program(d['A'], d['b'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], d['F'], equality_indices=list(d['equality_indices']))
            return solve_mpqp(prog, mpqp_algorithm.combinatorial)
    raise KeyError(name)


def _grid_check(sol, sl, n=200, inner=1e-4):
    """Points of an n x n grid over the slice's box, lifted to theta_0 + U z and located (get_region_batch): a point inside polygon r by
    more than ``inner`` (relative to the box) is located in r; a point located in r lies in polygon r within that margin; and the
    summed areas agree with the located share of the grid within the grid's boundary error."""
    from matplotlib.path import Path
    lo0, lo1, hi0, hi1 = sl.box
    g0, g1 = numpy.meshgrid(lo0 + (numpy.arange(n) + 0.5) * (hi0 - lo0) / n, lo1 + (numpy.arange(n) + 0.5) * (hi1 - lo1) / n)
    Z = numpy.stack([g0.ravel(), g1.ravel()], axis=1)
    loc = sol.get_region_batch(sl.lift(Z))
    D = numpy.hypot(hi0 - lo0, hi1 - lo1)
    full = numpy.flatnonzero(sl.full())
    inside_any = numpy.zeros(len(Z), dtype=bool)
    for r in full:
        V = sl.vertices[r]
        deep = Path(V).contains_points(Z, radius=-inner * D) | Path(V[::-1]).contains_points(Z, radius=-inner * D)
        wide = Path(V).contains_points(Z, radius=inner * D) | Path(V[::-1]).contains_points(Z, radius=inner * D)
        inside_any |= deep
        if not sol.is_overlapping:
            bad_in = numpy.flatnonzero(deep & (loc != r))
            assert len(bad_in) == 0, (int(r), len(bad_in), Z[bad_in[:3]], loc[bad_in[:3]])
        bad_out = numpy.flatnonzero((loc == r) & ~wide)
        assert len(bad_out) == 0, (int(r), len(bad_out), Z[bad_out[:3]])
    box_area = (hi0 - lo0) * (hi1 - lo1)
    located = numpy.count_nonzero(loc >= 0) / len(Z) * box_area
    perimeter = sum(numpy.sum(numpy.linalg.norm(numpy.roll(sl.vertices[r], -1, axis=0) - sl.vertices[r], axis=1)) for r in full)
    cell = max(hi0 - lo0, hi1 - lo1) / n
    assert abs(numpy.sum(sl.areas[full]) - located) <= perimeter * cell + 1e-9 * box_area, (numpy.sum(sl.areas[full]), located)
    return int(numpy.count_nonzero(loc >= 0))


def _regions_against_reference(sol, sl, every=1):
    for r in range(0, len(sol.critical_regions), every):
        cr = sol.critical_regions[r]
        E, f = numpy.asarray(cr.E, dtype=float), numpy.asarray(cr.f, dtype=float).reshape(-1)
        want = ref.slice_polygon(E, f, sl.theta_0, sl.U, sl.box)
        assert (sl.status[r] & ~ref.CUT) == (want['status'] & ~ref.CUT) or want['status'] == ref.LOWDIM or sl.status[r] == ref.LOWDIM, \
            (r, int(sl.status[r]), want['status'])
        if (sl.status[r] & ~ref.CUT) == ref.FULL and (want['status'] & ~ref.CUT) == ref.FULL:
            assert sl.status[r] == want['status'], (r, int(sl.status[r]), want['status'])
            D = numpy.hypot(sl.box[2] - sl.box[0], sl.box[3] - sl.box[1])
            assert len(sl.vertices[r]) == len(want['vertices']), (r, len(sl.vertices[r]), len(want['vertices']))
            assert numpy.max(numpy.abs(sl.vertices[r] - want['vertices'])) <= 1e-9 * D, r
            assert abs(sl.areas[r] - want['area']) <= 1e-9 * want['area'] + 1e-12 * D * D, r
            for q, row in enumerate(sl.edge_rows[r]):
                assert int(row) in want['edge_rows'][q], (r, q, int(row), want['edge_rows'][q])


@pytest.mark.parametrize('name', ['c1', 'c2', 'rand_4_2_10'])
def test_two_parameter_solutions(name):
    sol = _solve(name)
    assert sol.theta_dim() == 2
    # c1's parameter set after presolve is open (its theta >= 0 rows are redundant for the program): the box of the original data
    sl = sol.slice_2d(box=(0.0, 0.0, 1000.0, 1000.0) if name == 'c1' else None)
    assert len(sl) == len(sol.critical_regions) and numpy.count_nonzero(sl.full()) >= 1
    _regions_against_reference(sol, sl)
    assert _grid_check(sol, sl) > 0


@pytest.mark.parametrize('name, every', [('rand_5_3_8_s3', 1), ('c3', 50)])
def test_slices_of_solutions_with_more_parameters(name, every):
    sol = _solve(name)
    n_t = sol.theta_dim()
    assert n_t > 2
    # the middle of the parameter set's bounding box for the fixed parameters
    P = sol.program
    fixed = {}
    for t in range(2, n_t):
        c = numpy.zeros(n_t); c[t] = 1.0
        st, x, obj, _ = _lib.lp_solve_batch(numpy.asarray(P.A_t, float), numpy.asarray(P.b_t, float).reshape(-1), numpy.vstack([c, -c]),
                                            numpy.zeros((2, len(P.b_t)), dtype=numpy.uint8))
        fixed[t] = 0.5 * (obj[0] - obj[1]) * 0.3
    sl = sol.slice_2d(dims=(0, 1), fixed=fixed)
    assert numpy.count_nonzero(sl.full()) >= 1
    _regions_against_reference(sol, sl, every)
    assert _grid_check(sol, sl) > 0
    # an arbitrary plane through the same point
    rng = numpy.random.default_rng(1)
    Q, _ = numpy.linalg.qr(rng.standard_normal((n_t, 2)))
    sl2 = sol.slice_2d(plane=(sl.theta_0, Q * 0.5))
    _grid_check(sol, sl2)


def test_slice_1d_of_a_solution():
    sol = _solve('c2')
    rng = numpy.random.default_rng(2)
    u = rng.standard_normal(2)
    ls = sol.slice_1d(numpy.zeros(2), u)
    for r in range(len(ls)):
        cr = sol.critical_regions[r]
        ta, tb, st = ref.slice_interval(numpy.asarray(cr.E, float), numpy.asarray(cr.f, float).reshape(-1), numpy.zeros(2), u, ls.t_range)
        assert (ls.status[r] & ~ref.CUT) == (st & ~ref.CUT), r
        if (st & ~ref.CUT) == ref.FULL:
            assert numpy.allclose(ls.intervals[r], [ta, tb], rtol=0, atol=1e-9)
            x_a = cr.evaluate(numpy.array([[ta * u[0]], [ta * u[1]]])).ravel()
            assert numpy.allclose(ls.x_start[r], x_a, rtol=0, atol=1e-8)
    # the covered part of the line is the located part of a fine sample of it
    t = numpy.linspace(*ls.t_range, 2001)[1:-1]
    loc = sol.get_region_batch(t[:, None] * u[None, :])
    covered = sum(ls.intervals[r, 1] - ls.intervals[r, 0] for r in numpy.flatnonzero(ls.full()))
    assert abs(covered - numpy.count_nonzero(loc >= 0) / len(t) * (ls.t_range[1] - ls.t_range[0])) <= 0.01 * (ls.t_range[1] - ls.t_range[0])


def test_plots_end_to_end(tmp_path):
    import matplotlib
    matplotlib.use('Agg')
    from ppopt_amd import plot
    sol = _solve('c2')
    plot.parametric_plot(sol, save_path=str(tmp_path / 'c2'), show=False, seed=0)
    assert (tmp_path / 'c2.png').stat().st_size > 1000
    verts = plot.gen_vertices(sol)
    assert len(verts) == len(sol.critical_regions) and sum(len(v) >= 3 for v in verts) >= 1
    sol3 = _solve('rand_5_3_8_s3')
    plot.parametric_plot(sol3, save_path=str(tmp_path / 'r3'), show=False, seed=0, fixed={2: 0.0})
    assert (tmp_path / 'r3.png').stat().st_size > 1000
    plot.parametric_plot_1D(sol, save_path=str(tmp_path / 'line'), show=False, theta_0=numpy.zeros(2), direction=numpy.array([1.0, 0.3]))
    assert (tmp_path / 'line.png').stat().st_size > 1000
