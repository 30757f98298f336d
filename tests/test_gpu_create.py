"""The decisions of handle creation (ppopt_amd/csrc/create.hpp), on the smallest programs that reach each of its branches: which
engine the levels run on (Engine.engine_kind), the LDS bytes of the two LDS-engine layouts (recomputed here from the layout formula),
and which of the program's one-off blocks exist.  The expectations are written from creation's rules: the n_theta class by n_t (4, 8,
10, none above 10), one or two row slots by the live rows (<= 64, <= 128, none above), the column class by the dictionary's
n_x + n_t - n_eq columns (<= 14, <= 30, none above); a register path needs the vertex of the parameter set and the dictionary at a
nondegenerate vertex of the base polytope, which the seeds below give."""
import warnings

import numpy
import pytest

from ppopt_amd import MPQP_Program
from ppopt_amd._lib import Engine

pytestmark = pytest.mark.gpu

KKT_THREAD_MAX = 10


def program(n_x, n_t, m, seed, n_tc_extra=0, theta='box', n_eq=0, lp=False, c_scale=1.0):
    """Strictly convex QP (lp: an LP), m random dense rows and a box |x_i| <= 5; theta in [-1, 1]^n_t:
    'box': as 2 n_t parameter rows (+ n_tc_extra copies of them shifted outwards, never tight);
    'lower': the lower bounds as the n_t parameter rows, the upper ones as main rows (a pointed cone of parameter rows);
    'none': both as main rows, no parameter row.  n_eq = 1: the first dense row is an equality through the origin.  c_scale: a larger
    linear cost pushes the unconstrained optimum out of the feasible set (more than the one region of the empty active set)."""
    rng = numpy.random.default_rng(seed)
    A = numpy.vstack([rng.normal(size=(m, n_x)), numpy.eye(n_x), -numpy.eye(n_x)])
    F = numpy.vstack([0.3 * rng.normal(size=(m, n_t)), numpy.zeros((2 * n_x, n_t))])
    b = numpy.concatenate([1.0 + numpy.abs(F[:m]).sum(axis=1) + rng.uniform(0.5, 1.5, size=m), numpy.full(2 * n_x, 5.0)])
    if n_eq:
        b[0] = 0.0
    I = numpy.eye(n_t)
    A_t, b_t = numpy.vstack([I, -I]), numpy.ones(2 * n_t)
    if n_tc_extra:
        idx = numpy.arange(n_tc_extra) % (2 * n_t)
        A_t = numpy.vstack([A_t, A_t[idx]])
        b_t = numpy.concatenate([b_t, 1.0 + 0.01 * (1 + numpy.arange(n_tc_extra))])
    if theta != 'box':   # theta_j <= 1 (and, for 'none', -theta_j <= 1) as main rows: A x - F theta <= b with a zero row of A
        rows = [I] if theta == 'lower' else [I, -I]
        for R in rows:
            A = numpy.vstack([A, numpy.zeros((n_t, n_x))]); F = numpy.vstack([F, -R]); b = numpy.concatenate([b, numpy.ones(n_t)])
        A_t, b_t = (-I, numpy.ones(n_t)) if theta == 'lower' else (numpy.zeros((0, n_t)), numpy.zeros(0))
    M = rng.normal(size=(n_x, n_x))
    Q = None if lp else M @ M.T + n_x * numpy.eye(n_x)
    return dict(A=A, b=b, F=F, c=c_scale * rng.normal(size=n_x), H=0.1 * rng.normal(size=(n_x, n_t)), Q=Q, A_t=A_t, b_t=b_t, n_eq=n_eq)


def engine(d):
    return Engine(d['A'], d['b'], d['F'], d['c'], d['H'], d['Q'], d['A_t'], d['b_t'], d['n_eq'])


def layout_bytes(size_T, size_K, size_L, size_E, size_X, kmax, n_c, ld_max, rows_max, rows_t):
    """make_layout: five areas of doubles, each rounded up to an even count, then eight integer arrays, 16-byte granularity"""
    doubles = sum((s + 1) & ~1 for s in (size_T, size_K, size_L, size_E, size_X))
    ints = (kmax + 1) + (n_c + 1) + (ld_max + 2) + 3 * (rows_max + 3) + 2 * (rows_t + 1)
    return (doubles * 8 + ints * 4 + 15) & ~15


def expected_lds(d, kkt_mode):
    odd = lambda v: v if v % 2 else v + 1
    (n_c, n_x), n_t, n_tc, n_eq = d['A'].shape, d['F'].shape[1], d['A_t'].shape[0], d['n_eq']
    nr, kmax, rows_x, rows_t = n_t + 1, min(n_c, n_x), n_c + n_tc, n_c - n_eq + n_tc
    ld_x, ld_t = odd(n_x + n_t + 3), odd(n_t + 4)
    size_K = max(kmax * kmax + kmax, kmax * n_x) if kkt_mode == 0 else max((n_x + kmax) ** 2 + (n_x + kmax) * nr, kmax * n_x, n_x * n_x)
    size_L, size_X = max(kmax * nr, 1), n_x * nr
    lds_v = layout_bytes(max((rows_x + 1) * ld_x, (rows_t + 1) * ld_t), size_K, size_L, 0, size_X if kkt_mode == 1 else 0, kmax, n_c, max(ld_x, ld_t), rows_x + 1, rows_t)
    lds_r = layout_bytes(max((rows_t + 2) * ld_t, rows_t * nr), size_K, size_L, rows_t * nr, size_X, kmax, n_c, ld_t, rows_t + 2, rows_t)
    return lds_v, lds_r


def expected_kind(d, env=()):
    """engine_kind by creation's rules, for a program whose base vertex is nondegenerate (the dictionary is built)"""
    (n_c, n_x), n_t, n_tc, n_eq = d['A'].shape, d['F'].shape[1], d['A_t'].shape[0], d['n_eq']
    slots = lambda rows: 1 if rows <= 64 else (2 if rows <= 128 else 0)
    rows_t = n_c - n_eq + n_tc
    s_t, s_x, s_r = slots(rows_t - n_t), slots(n_c + n_tc - (n_x + n_t)), slots(rows_t + 1)
    nt_class = 4 if n_t <= 4 else (8 if n_t <= 8 else (10 if n_t <= 10 else 0))
    columns = n_x + n_t - n_eq
    has_vertex = n_tc >= n_t     # (of the parameter set: the box and the pointed cone have one)
    fast = bool(has_vertex and s_t and s_x and nt_class and columns <= 30 and 'MPC_FORCE_V1' not in env)
    kkt_mode = 1 if d['Q'] is None else 0
    # open: no parameter row, or the cone of the lower bounds alone
    return {'register_engine': fast, 'rows_per_lane_theta': s_t if fast else 0, 'rows_per_lane_x': s_x if fast else 0,
            'rows_per_lane_region': s_r if fast and n_t >= 2 else 0, 'n_theta_instantiation': nt_class if fast else 0,
            'theta_open': n_tc < 2 * n_t, 'kkt_mode': kkt_mode,
            'kkt_thread_max_rows': KKT_THREAD_MAX if fast and kkt_mode == 0 and 'MPC_NO_KKT_THREAD' not in env else 0}


def block_sizes(e):
    return [e.program_block(w).size for w in range(11)]


def expected_blocks(d, env=()):
    (n_c, n_x), nr, n_eq = d['A'].shape, d['F'].shape[1] + 1, d['n_eq']
    schur = [n_c * n_c, n_c * nr, n_c * n_x, n_x * nr] if d['Q'] is not None else [0, 0, 0, 0]
    elim = n_eq > 0 and d['Q'] is not None and 'MPC_NO_EQ_ELIM' not in env
    return schur + [n_c * n_c] + ([n_c * n_c, n_c * nr, n_c * n_c, n_eq * nr, n_eq * n_c, 2 * n_eq] if elim else [0] * 6)


# name: (program arguments, environment, what the case reaches)
CASES = {
    'nt2': (dict(n_x=3, n_t=2, m=4, seed=1), {}, 'NT class 4, one slot everywhere, column class 0'),
    'nt5': (dict(n_x=3, n_t=5, m=4, seed=2), {}, 'NT class 8'),
    'nt9': (dict(n_x=3, n_t=9, m=4, seed=3), {}, 'NT class 10'),
    'nt11': (dict(n_x=3, n_t=11, m=4, seed=4), {}, 'no register path above n_t = 10'),
    'theta_rows_72': (dict(n_x=3, n_t=2, m=4, seed=1, n_tc_extra=60), {}, 'live theta rows 72 > 64: two slots (theta, x and region)'),
    'theta_rows_142': (dict(n_x=3, n_t=2, m=4, seed=1, n_tc_extra=130), {}, 'live theta rows 142 > 128: LDS-engine kernels'),
    'columns_16': (dict(n_x=14, n_t=2, m=4, seed=5), {}, 'dictionary of 16 columns: column class 1'),
    'columns_32': (dict(n_x=30, n_t=2, m=4, seed=6), {}, 'dictionary of 32 columns: no register path'),
    'cone': (dict(n_x=3, n_t=2, m=4, seed=7, theta='lower'), {}, 'n_tc == n_t, independent lower bounds: a vertex without an LP, open set'),
    'no_theta_rows': (dict(n_x=3, n_t=2, m=4, seed=8, theta='none'), {}, 'n_tc == 0: no vertex, open set'),
    'equality': (dict(n_x=3, n_t=2, m=4, seed=9, n_eq=1), {}, 'an equality row, eliminated from the Schur blocks: blocks 5..10'),
    'equality_no_elim': (dict(n_x=3, n_t=2, m=4, seed=9, n_eq=1), {'MPC_NO_EQ_ELIM': '1'}, '... not eliminated: blocks 5..10 empty'),
    'lp': (dict(n_x=3, n_t=2, m=4, seed=10, lp=True), {}, 'no Q: kkt_mode 1, blocks 0..3 empty'),
    'nc130': (dict(n_x=3, n_t=2, m=124, seed=11), {}, 'n_c = 130: four-word masks (and 132 live theta rows: LDS-engine kernels)'),
    'force_v1': (dict(n_x=3, n_t=2, m=4, seed=1), {'MPC_FORCE_V1': '1'}, 'register path switched off'),
    'no_kkt_thread': (dict(n_x=3, n_t=2, m=4, seed=1), {'MPC_NO_KKT_THREAD': '1'}, 'no KKT thread kernel'),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_creation_decisions(name, monkeypatch):
    args, env, _ = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = program(**args)
    e = engine(d)
    try:
        kind = e.engine_kind()
        lds = (e.lds_bytes(0), e.lds_bytes(1))
        blocks = block_sizes(e)
        print(name, kind, lds, blocks, e.mask_words)
        assert kind == expected_kind(d, env)
        assert max(lds) <= 160 * 1024 and lds == expected_lds(d, kind['kkt_mode'])
        assert blocks == expected_blocks(d, env)
        assert e.mask_words == (4 if d['A'].shape[0] > 128 else 2)
    finally:
        e.close()


def test_box_select_form_solves_to_the_same_regions(monkeypatch):
    """MPC_KKT_BOX_SELECT=1 only changes the form of a screen's row test: creation makes the same decisions, the solve gives the same regions"""
    from ppopt_amd.mp_solvers import mpqp_hip_combinatorial
    d = program(n_x=3, n_t=5, m=4, seed=2, c_scale=30.0)    # (four regions: the CPU oracle's count)
    out = []
    for select in (False, True):
        if select:
            monkeypatch.setenv('MPC_KKT_BOX_SELECT', '1')
        e = engine(d)
        out.append((e.engine_kind(), e.lds_bytes(0), e.lds_bytes(1), block_sizes(e)))
        e.close()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            prog = MPQP_Program(d['A'], d['b'].reshape(-1, 1), d['c'].reshape(-1, 1), d['H'], d['Q'], d['A_t'], d['b_t'].reshape(-1, 1), d['F'])
            sol = mpqp_hip_combinatorial.solve(prog)
        out.append({tuple(r.active_set): r for r in sol.critical_regions})
    assert out[0] == out[2] and out[0][0]['register_engine']
    assert len(out[1]) == 4 and sorted(out[1]) == sorted(out[3])
    for key, r in out[1].items():       # same index sets, coefficients within the 1e-8 the regions are compared with everywhere (smoke, parity)
        q = out[3][key]
        assert (r.omega_set, r.lambda_set, r.regular_set) == (q.omega_set, q.lambda_set, q.regular_set), key
        for u, v in ((r.A, q.A), (r.b, q.b), (r.C, q.C), (r.d, q.d)):
            assert numpy.max(numpy.abs(u - v) / (1 + numpy.abs(v))) <= 1e-8, key
