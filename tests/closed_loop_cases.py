"""The cases of the exact closed-loop tests: synthetic partitions, lattice laws and plants, and their exact references.
tests/test_closed_loop_cpu.py checks on the host that every case is exact and exercises what it is meant to exercise;
tests/test_gpu_closed_loop_exact.py runs the same cases on the device.  A plain helper module (not a conftest); nothing of ppopt_amd is
imported here."""
import functools

import numpy

import closed_loop_reference as ref
import locate_reference as lref

TOL = lref.TOL
N_TRAJ, STEPS = 400, 8
RULES_TOL = 0.125
_SIX = numpy.arange(7) - 3.0

# n_theta: (cuts, bases with two mask words / n_c 128, bases with four mask words / n_c 256).  The same cells are built with both: the
# two-word ids straddle bits 63 / 64, the four-word ids lie in words 2 and 3 (word 1 too at n_theta 4, 8 and 9).
GRID_SHAPES = {
    1: ({0: numpy.arange(13) * 0.5 - 3.0}, {0: 58}, {0: 186}),
    4: ({0: _SIX, 3: _SIX}, {0: 61, 3: 100}, {0: 125, 3: 189}),
    5: ({0: numpy.arange(6) - 2.5, 1: numpy.arange(5) - 2.0, 2: numpy.arange(4) * 2.0 - 3.0}, {0: 61, 1: 0, 2: 126}, {0: 189, 1: 130, 2: 254}),
    8: ({1: _SIX, 7: _SIX}, {1: 61, 7: 100}, {1: 125, 7: 189}),
    9: ({2: _SIX, 8: _SIX}, {2: 61, 8: 100}, {2: 125, 8: 189}),
    16: ({3: _SIX, 15: _SIX}, {3: 61, 15: 120}, {3: 130, 15: 250}),
}


def grids(n_t):
    cuts, b2, b4 = GRID_SHAPES[n_t]
    return lref.Grid(n_t, cuts, b2, 128, 2), lref.Grid(n_t, cuts, b4, 256, 4)


def planes_of(row_off, ef):
    """(planes [H, n_t + 1] unit [n | o], cand_off, cand_plane): every distinct hyperplane of the rows once, its first non-zero
    coefficient positive, and the planes of every region -- what SearchTree.build hands to mpc_tree_build"""
    n_t = ef.shape[1] - 1
    index, planes, cand_off, cand_plane = {}, [], [0], []
    for r in range(len(row_off) - 1):
        for row in ef[row_off[r]:row_off[r + 1]]:
            norm = float(numpy.linalg.norm(row[1:]))
            if norm == 0.0:
                continue
            unit = numpy.r_[row[1:], row[0]] / norm
            if unit[numpy.flatnonzero(unit[:n_t])[0]] < 0:
                unit = -unit
            key = tuple(numpy.round(unit, 9) + 0.0)
            if key not in index:
                index[key] = len(planes)
                planes.append(unit)
            cand_plane.append(index[key])
        cand_off.append(len(cand_plane))
    return numpy.array(planes).reshape(len(planes), n_t + 1), numpy.array(cand_off, dtype=numpy.int64), numpy.array(cand_plane, dtype=numpy.int32)


def _grid_case(n_t, n_u, with_c, with_w, stop_tol, seed, n=N_TRAJ, steps=STEPS, holes=False, n_x=None, diag=0.5, reach=3.5):
    """A closed loop over the cells of the grid of n_theta, in shuffled order; `holes`: some cells are missing and some have rows of
    unknown kind (the walk cannot cross them)."""
    rng = numpy.random.default_rng(seed)
    g2, g4 = grids(n_t)
    cells = g2.shuffled(seed)
    unknown = set()
    if holes:
        gone = set(cells[3::11])
        cells = [cell for cell in cells if cell not in gone]
        unknown = set(cells[2::7])
    b2, b4 = g2.build(cells, unknown=unknown), g4.build(cells, unknown=unknown)
    n_x = n_x or (20 if n_u > 5 else 17)
    case = {'n_t': n_t, 'n_u': n_u, 'n_x': n_x, 'n': n, 'steps': steps, 'tol': TOL, 'band': 16.0 * TOL, 'stop_tol': stop_tol, 'flags': {},
            'row_off': b2['row_off'], 'ef': b2['ef'], 'xlaw': ref.lattice_laws(rng, len(cells), n_x, n_t), 'Q': None, 'cvec': None, 'H': None,
            'walk2': (b2['masks'], b2['row_info'], 128), 'walk4': (b4['masks'], b4['row_info'], 256)}
    case.update(ref.lattice_plant(rng, n_t, n_u, n_x, with_c, diag))
    case['theta0'] = ref.lattice_starts(rng, n, n_t, TOL, reach)
    case['w'] = ref.lattice_disturbance(rng, n, steps, n_t) if with_w else None
    return case


def _rules_case(n_t, flags, seed, n=N_TRAJ, steps=3):
    """Overlapping boxes with oblique rows, one region without rows, and the objective of locate_reference.lattice_case.  A = I, B has
    one entry of +-1/8 in four of its rows, and the starts lie on the 1/8 lattice, most of them inside a box: the objective of three steps then
    stays within 53 bits (each step refines the lattice of theta by five bits, and the objective squares it; a fourth step would need
    about ten bits more).  The tolerance is 1/8, a lattice step, so that starts exactly tol beyond a row exist and the strict and the
    inclusive rule part; the tree's band stays 2^-10, since the band covers the rounding of the builder's LPs, not the tolerance."""
    row_off, ef, xlaw, Q, cvec, H, _ = lref.lattice_case(seed, n_t, 3, True)
    rng = numpy.random.default_rng(seed + 1)
    B = numpy.zeros((n_t, 2))
    moved = rng.permutation(n_t)[:4]     # four coordinates move, the others keep their start
    B[moved, rng.integers(0, 2, size=4)] = rng.choice([-0.125, 0.125], size=4)
    boxed = [r for r in range(len(row_off) - 1) if row_off[r + 1] > row_off[r]]
    theta0 = lref.lattice(rng, (n, n_t), -3.5, 3.5, RULES_TOL)
    for p in range(n - n // 8):     # inside a box: its lower corner plus up to 2 (rows 2a, 2a + 1 of a box: theta_a <= hi_a, -theta_a <= -lo_a)
        rows = ef[row_off[boxed[int(rng.integers(len(boxed)))]]:][:2 * n_t]
        theta0[p] = -rows[1::2, 0] + lref.lattice(rng, n_t, 0.0, 2.0, RULES_TOL)
        if p % 8 == 0:              # exactly tol beyond one upper row: outside by the strict rule, inside by the inclusive one
            a = int(rng.integers(n_t))
            theta0[p, a] = rows[2 * a, 0] + RULES_TOL
    return {'n_t': n_t, 'n_u': 2, 'n_x': 3, 'n': n, 'steps': steps, 'tol': RULES_TOL, 'band': TOL, 'stop_tol': None, 'flags': dict(flags),
            'row_off': row_off, 'ef': ef, 'xlaw': xlaw, 'Q': Q, 'cvec': cvec, 'H': H, 'A': numpy.eye(n_t), 'B': B, 'c': None,
            'inputs': [2, 0], 'theta0': theta0[rng.permutation(n)], 'w': None}


# name: (n_theta, n_u, c, w, stop_tol, diagonal of A, reach of the starts).  Width cases w<n_theta>u<n_u>: both edges of every theta
# width (4 / 8 / 16) with both input widths (4 / 16), n_x = 17 or 20, every combination of c and w, a stop tolerance at every theta width.
_WIDTHS = {
    'w1u1': (1, 1, False, True, None, 1.0, 3.0), 'w1u5': (1, 5, True, False, 0.125, 1.0, 3.0),
    'w4u4': (4, 4, False, True, None, 0.75, 3.0), 'w4u16': (4, 16, True, True, None, 0.75, 3.0),
    'w5u5': (5, 5, False, False, 0.125, 0.75, 2.5), 'w5u4': (5, 4, True, False, None, 0.75, 2.5),
    'w8u16': (8, 16, False, True, None, 0.75, 3.0), 'w8u1': (8, 1, True, True, None, 0.75, 3.0),
    'w9u4': (9, 4, False, False, 0.125, 0.5, 3.0), 'w9u5': (9, 5, True, False, None, 0.75, 3.0),
    'w16u1': (16, 1, False, True, None, 0.75, 3.0), 'w16u16': (16, 16, True, True, None, 0.75, 3.0),
}
WIDTH_CASES = list(_WIDTHS)
_BUILDERS = {}
for _i, (_name, (_nt, _nu, _c, _w, _stop, _diag, _reach)) in enumerate(_WIDTHS.items()):
    _BUILDERS[_name] = functools.partial(_grid_case, _nt, _nu, _c, _w, _stop, 100 + _i, diag=_diag, reach=_reach)
COUNTS = [1, 63, 64, 65, 255, 256, 257, 513]
_BUILDERS['counts'] = functools.partial(_grid_case, 4, 4, True, True, None, 200, n=COUNTS[-1], steps=6, diag=0.75, reach=3.0)
_BUILDERS['holes'] = functools.partial(_grid_case, 5, 4, True, True, None, 201, holes=True, diag=0.5, reach=2.0)
RULE_FLAGS = {'overlapping': dict(overlapping=True), 'inclusive': dict(inclusive=True), 'both': dict(overlapping=True, inclusive=True)}
RULES_CASES = [f'rules{n_t}_{name}' for n_t in (4, 9) for name in RULE_FLAGS]
for _name in RULES_CASES:
    _nt, _rule = int(_name[5:_name.index('_')]), _name.split('_')[1]
    # three steps are what the objective's certificate allows; without an objective there is room for five
    _BUILDERS[_name] = functools.partial(_rules_case, _nt, RULE_FLAGS[_rule], {4: 302, 9: 322}[_nt], steps=5 if _rule == 'inclusive' else 3)
LATTICE_CASES = WIDTH_CASES + ['counts', 'holes'] + RULES_CASES


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the exact reference of a case, computed once; nobody writes to it"""
    k = case(name)
    out = ref.simulate_rows(k['row_off'], k['ef'], k['xlaw'], k['theta0'], k['steps'], k['A'], k['B'], k['inputs'], k['c'], k['w'], k['tol'],
                            k['stop_tol'], Q=k['Q'], cvec=k['cvec'], H=k['H'], **k['flags'])
    for v in out.values():
        if isinstance(v, numpy.ndarray):
            v.setflags(write=False)
    return out


def quality(out, steps):
    """What a reference run exercises: dict of bits, the share of trajectories that run every step, the number that find no region at
    a step >= 1, the number that end steady, the share of consecutive step pairs in which the region changes, and the largest number of
    different exit steps before the last in a block of 256 trajectories in which some trajectory runs to the end."""
    st, ex, reg = out['status'], out['exit_step'], out['region']
    both = (reg[:, 1:] >= 0) & (reg[:, :-1] >= 0)
    staggered = 0
    for b0 in range(0, len(st), 256):
        s, e = st[b0:b0 + 256], ex[b0:b0 + 256]
        if (s == 0).any():
            staggered = max(staggered, len(set(e[e < steps])))
    return {'bits': out['bits'], 'full': float(numpy.mean(st == 0)), 'lost_later': int(numpy.sum((st == 2) & (ex >= 1))),
            'lost_at_start': int(numpy.sum((st == 2) & (ex == 0))), 'steady': int(numpy.sum(st == 1)),
            'changes': float(numpy.sum(reg[:, 1:][both] != reg[:, :-1][both]) / max(1, both.sum())), 'staggered': staggered,
            'regions': len(numpy.unique(reg[reg >= 0]))}
