"""The host side the pair-stage calls share (ppopt_amd/_pairs.py), without a device: every refusal of the seven callers
word for word and in its order, the one sweep core against the numpy reference of box_pairs_reference.py, and the keys of ``stats`` that
the three callers of candidate_pairs report with the host sweep and no screen."""
import sys

import numpy
import pytest

import box_pairs_reference as ref
from ppopt_amd import Solution, _cells, _lib, _pairs, compare, exit_sets, overlap, transition
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.geometry import box_pairs as _bp_function      # noqa: F401  (loads the module; the package exports the function under its name)
from ppopt_amd.geometry import reduce as reduce_module

bp = sys.modules['ppopt_amd.geometry.box_pairs']

TOL = ref.TOL
INF, NAN = numpy.inf, numpy.nan
SQUARE = numpy.array([[1.0, 1.0, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 0.0, -1.0]])      # unit rows [o | n] of [0, 1]^2


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', refuse)


# ---- 1. the refusals ---------------------------------------------------------------------------------------------------------------------------
def good():
    """two unit squares at n_theta = 2: the smallest input that passes every check"""
    box = numpy.tile(numpy.array([[0.0, 0.0], [1.0, 1.0]]), (2, 1, 1))
    return dict(off=numpy.array([0, 4, 8]), ef=numpy.vstack([SQUARE, SQUARE]), n_t=2, tol=1e-8, Phi=numpy.tile(numpy.eye(2), (2, 1, 1)), phi=numpy.zeros((2, 2)),
                g=numpy.zeros((2, 2)), h=numpy.zeros(2), laws=numpy.zeros((2, 1, 3)), pa=[0], pb=[1], box=box, max_pieces=4, max_steps=8, sides='both')


CALLS = {
    'partition_by_value': lambda a: overlap.partition_by_value(a['off'], a['ef'], a['g'], a['h'], a['n_t'], tol=a['tol']),
    'transition_pairs': lambda a: transition.transition_pairs(a['off'], a['ef'], a['Phi'], a['phi'], a['n_t'], tol=a['tol'], pairs=(a['pa'], a['pb'])),
    'law_gap_pairs': lambda a: compare.law_gap_pairs(a['off'], a['ef'], a['laws'], a['pa'], a['pb'], tol=a['tol']),
    'exit_pieces': lambda a: exit_sets.exit_pieces(a['off'], a['ef'], a['Phi'], a['phi'], a['n_t'], [[], []], tol=a['tol'], max_pieces=a['max_pieces']),
    'screen_pairs': lambda a: bp.screen_pairs(a['off'], a['ef'], a['pa'], a['pb'], a['box'], a['box'], sides=a['sides']),
    'reduce_rows_of': lambda a: reduce_module.reduce_rows_of(a['off'], a['ef'], a['n_t'], tol=a['tol']),
    'cells': lambda a: _cells.check_cell_call('cells', a['off'], a['ef'], a['Phi'], a['phi'], a['n_t'], 'predecessors', [[], []], [0], numpy.zeros((0, 3)),
                                              'cell_source', 'one source', [], a['tol'], a['max_steps'], 16, None),
}


def _rows(n):
    """[0, n, n + 4] and the rows of a first polytope of n rows (the square's, repeated) before the second square"""
    return numpy.array([0, n, n + 4]), numpy.vstack([numpy.tile(SQUARE, (n // 4 + 1, 1))[:n], SQUARE])


def _nan_row(a):
    ef = a['ef'].copy()
    ef[5, 0] = NAN
    return dict(ef=ef)


SPOILS = {
    'n_t = 0': lambda a: dict(n_t=0),
    'n_t = 17': lambda a: dict(n_t=17),
    '18 columns': lambda a: dict(ef=numpy.zeros((8, 18))),
    'tol = -1': lambda a: dict(tol=-1.0),
    'tol = nan': lambda a: dict(tol=NAN),
    'off[0] = 1': lambda a: dict(off=numpy.array([1, 4, 8])),
    'off[-1] = 9': lambda a: dict(off=numpy.array([0, 4, 9])),
    'empty polytope': lambda a: dict(off=numpy.array([0, 0, 8])),
    '257 rows': lambda a: dict(zip(('off', 'ef'), _rows(257))),
    '513 rows': lambda a: dict(zip(('off', 'ef'), _rows(513))),
    'nan row': _nan_row,
    'long row': lambda a: dict(ef=a['ef'] * 2.0),
    'Phi shape': lambda a: dict(Phi=a['Phi'][:1]),
    'phi shape': lambda a: dict(phi=a['phi'][:, :1]),
    'Phi nan': lambda a: dict(Phi=a['Phi'] * NAN),
    'phi nan': lambda a: dict(phi=a['phi'] + NAN),
    'g shape': lambda a: dict(g=numpy.zeros((3, 2))),
    'h shape': lambda a: dict(h=numpy.zeros(3)),
    'g nan': lambda a: dict(g=a['g'] + NAN),
    'h nan': lambda a: dict(h=a['h'] + NAN),
    'laws shape': lambda a: dict(laws=numpy.zeros((2, 1, 4))),
    'laws nan': lambda a: dict(laws=a['laws'] + NAN),
    'pairs of unequal length': lambda a: dict(pa=[0, 1]),
    'pair -1': lambda a: dict(pb=[-1]),
    'pair R': lambda a: dict(pa=[2]),
    'max_pieces = 0': lambda a: dict(max_pieces=0),
    'max_steps = -1': lambda a: dict(max_steps=-1),
    "sides = 'c'": lambda a: dict(sides='c'),
}

# the texts below are the f-strings of the source before _pairs.py, with the values of these inputs filled in
MAPS = 'row_off [R + 1], Phi [R, n_t, n_t] and phi [R, n_t] must describe R >= 1 polytopes'
VALUES = 'row_off [R + 1], g [R, n_t] and h [R] must describe R >= 1 polytopes'
TABLE = 'row_off [R + 1] must run from 0 to the number of rows of ef_rows [rows, n_t + 1] and describe R >= 1 polytopes'
REDUCE_TABLE = 'row_off [n + 1] must run from 0 to the number of rows and describe n >= 1 polytopes'
TOL_TEXT = 'tol must be finite and >= 0'
PAIRS = 'pair_a and pair_b must be two index arrays of one length into the polytopes'
ROWS_256, ROWS_512 = 'every polytope needs 1..256 rows', 'every polytope needs 1..512 rows'

REFUSALS = [      # (caller, what is spoiled: the first entry is what the refusal names, refusal without the caller's name)
    ('partition_by_value', ['n_t = 0'], 'n_theta = 0 is outside 1..16'), ('partition_by_value', ['n_t = 17'], 'n_theta = 17 is outside 1..16'),
    ('partition_by_value', ['tol = -1'], 'tol and value_tol must be finite and >= 0'), ('partition_by_value', ['tol = nan'], 'tol and value_tol must be finite and >= 0'),
    ('partition_by_value', ['off[0] = 1'], VALUES), ('partition_by_value', ['off[-1] = 9'], VALUES), ('partition_by_value', ['g shape'], VALUES),
    ('partition_by_value', ['h shape'], VALUES), ('partition_by_value', ['empty polytope'], ROWS_256), ('partition_by_value', ['257 rows'], ROWS_256),
    ('partition_by_value', ['nan row'], 'rows and values must be finite'), ('partition_by_value', ['g nan'], 'rows and values must be finite'),
    ('partition_by_value', ['h nan'], 'rows and values must be finite'),
    ('partition_by_value', ['n_t = 17', 'tol = -1'], 'n_theta = 17 is outside 1..16'), ('partition_by_value', ['tol = nan', 'off[0] = 1'], 'tol and value_tol must be finite and >= 0'),
    ('partition_by_value', ['off[0] = 1', 'nan row'], VALUES), ('partition_by_value', ['empty polytope', 'g nan'], ROWS_256),

    ('transition_pairs', ['n_t = 0'], 'n_theta = 0 is outside 1..16'), ('transition_pairs', ['n_t = 17'], 'n_theta = 17 is outside 1..16'),
    ('transition_pairs', ['tol = -1'], TOL_TEXT), ('transition_pairs', ['tol = nan'], TOL_TEXT), ('transition_pairs', ['off[0] = 1'], MAPS),
    ('transition_pairs', ['off[-1] = 9'], MAPS), ('transition_pairs', ['Phi shape'], MAPS), ('transition_pairs', ['phi shape'], MAPS),
    ('transition_pairs', ['empty polytope'], ROWS_256), ('transition_pairs', ['257 rows'], ROWS_256), ('transition_pairs', ['nan row'], 'rows and maps must be finite'),
    ('transition_pairs', ['Phi nan'], 'rows and maps must be finite'), ('transition_pairs', ['phi nan'], 'rows and maps must be finite'),
    ('transition_pairs', ['pairs of unequal length'], 'pairs must be two index arrays of one length into the polytopes'),
    ('transition_pairs', ['pair -1'], 'pairs must be two index arrays of one length into the polytopes'),
    ('transition_pairs', ['pair R'], 'pairs must be two index arrays of one length into the polytopes'),
    ('transition_pairs', ['n_t = 0', 'tol = -1'], 'n_theta = 0 is outside 1..16'), ('transition_pairs', ['tol = -1', 'off[0] = 1'], TOL_TEXT),
    ('transition_pairs', ['Phi shape', 'empty polytope'], MAPS), ('transition_pairs', ['nan row', 'pair -1'], 'rows and maps must be finite'),

    ('law_gap_pairs', ['18 columns'], 'n_theta = 17 is outside 1..16'), ('law_gap_pairs', ['tol = -1'], TOL_TEXT), ('law_gap_pairs', ['tol = nan'], TOL_TEXT),
    ('law_gap_pairs', ['off[0] = 1'], TABLE), ('law_gap_pairs', ['off[-1] = 9'], TABLE), ('law_gap_pairs', ['empty polytope'], ROWS_256),
    ('law_gap_pairs', ['257 rows'], ROWS_256), ('law_gap_pairs', ['nan row'], 'rows and laws must be finite'), ('law_gap_pairs', ['laws nan'], 'rows and laws must be finite'),
    ('law_gap_pairs', ['laws shape'], 'laws must be [2, K, 3] = [b | A], not [2, 1, 4]'), ('law_gap_pairs', ['pairs of unequal length'], PAIRS),
    ('law_gap_pairs', ['pair -1'], PAIRS), ('law_gap_pairs', ['pair R'], PAIRS),
    ('law_gap_pairs', ['off[0] = 1', '18 columns'], TABLE), ('law_gap_pairs', ['laws shape', 'tol = -1'], 'laws must be [2, K, 3] = [b | A], not [2, 1, 4]'),
    ('law_gap_pairs', ['tol = -1', 'empty polytope'], TOL_TEXT), ('law_gap_pairs', ['nan row', 'pair R'], 'rows and laws must be finite'),

    ('exit_pieces', ['n_t = 0'], 'n_theta = 0 is outside 1..16'), ('exit_pieces', ['n_t = 17'], 'n_theta = 17 is outside 1..16'), ('exit_pieces', ['tol = -1'], TOL_TEXT),
    ('exit_pieces', ['tol = nan'], TOL_TEXT), ('exit_pieces', ['max_pieces = 0'], 'max_pieces must be >= 1'), ('exit_pieces', ['off[0] = 1'], MAPS),
    ('exit_pieces', ['off[-1] = 9'], MAPS), ('exit_pieces', ['Phi shape'], MAPS), ('exit_pieces', ['phi shape'], MAPS), ('exit_pieces', ['empty polytope'], ROWS_256),
    ('exit_pieces', ['257 rows'], ROWS_256), ('exit_pieces', ['nan row'], 'rows and maps must be finite'), ('exit_pieces', ['Phi nan'], 'rows and maps must be finite'),
    ('exit_pieces', ['phi nan'], 'rows and maps must be finite'),
    ('exit_pieces', ['tol = -1', 'max_pieces = 0'], TOL_TEXT), ('exit_pieces', ['max_pieces = 0', 'off[0] = 1'], 'max_pieces must be >= 1'),
    ('exit_pieces', ['empty polytope', 'Phi nan'], ROWS_256),

    ('screen_pairs', ['off[0] = 1'], TABLE), ('screen_pairs', ['off[-1] = 9'], TABLE), ('screen_pairs', ['pairs of unequal length'], PAIRS),
    ('screen_pairs', ['pair -1'], PAIRS), ('screen_pairs', ['pair R'], PAIRS),
    ('screen_pairs', ["sides = 'c'", 'off[0] = 1'], "sides must be 'a', 'b' or 'both', not 'c'"), ('screen_pairs', ['off[0] = 1', 'pair -1'], TABLE),
    ('screen_pairs', ['18 columns', 'pair R'], 'n_theta = 17 is outside 1..16'),

    ('reduce_rows_of', ['n_t = 0'], 'n_theta = 0 is outside 1..16'), ('reduce_rows_of', ['n_t = 17'], 'n_theta = 17 is outside 1..16'),
    ('reduce_rows_of', ['tol = -1'], TOL_TEXT), ('reduce_rows_of', ['tol = nan'], TOL_TEXT), ('reduce_rows_of', ['18 columns'], 'ef_rows must be [rows, 3], not [8, 18]'),
    ('reduce_rows_of', ['off[0] = 1'], REDUCE_TABLE), ('reduce_rows_of', ['off[-1] = 9'], REDUCE_TABLE), ('reduce_rows_of', ['empty polytope'], ROWS_512),
    ('reduce_rows_of', ['513 rows'], ROWS_512), ('reduce_rows_of', ['nan row'], 'rows must be finite'),
    ('reduce_rows_of', ['tol = -1', 'off[0] = 1'], TOL_TEXT), ('reduce_rows_of', ['empty polytope', 'nan row'], ROWS_512),
    ('reduce_rows_of', ['nan row', 'long row'], 'rows must be finite'),

    ('cells', ['n_t = 0'], 'n_theta = 0 is outside 1..16'), ('cells', ['n_t = 17'], 'n_theta = 17 is outside 1..16'), ('cells', ['tol = -1'], TOL_TEXT),
    ('cells', ['tol = nan'], TOL_TEXT), ('cells', ['off[0] = 1'], MAPS), ('cells', ['off[-1] = 9'], MAPS), ('cells', ['Phi shape'], MAPS), ('cells', ['phi shape'], MAPS),
    ('cells', ['empty polytope'], ROWS_256), ('cells', ['257 rows'], ROWS_256), ('cells', ['nan row'], 'rows and maps must be finite'),
    ('cells', ['Phi nan'], 'rows and maps must be finite'), ('cells', ['phi nan'], 'rows and maps must be finite'),
    ('cells', ['tol = nan', 'max_steps = -1'], TOL_TEXT), ('cells', ['max_steps = -1', 'off[0] = 1'], 'max_steps must be >= 0'),
    ('cells', ['Phi shape', 'nan row'], MAPS),
]


@pytest.mark.parametrize('caller,spoiled,text', REFUSALS, ids=[f'{c}: {" and ".join(s)}' for c, s, _ in REFUSALS])
def test_refusals_word_for_word_and_in_order(no_library, caller, spoiled, text):
    args = good()
    for name in spoiled:
        args.update(SPOILS[name](args))
    with pytest.raises(ValueError) as err:
        CALLS[caller](args)
    assert str(err.value) == f'{caller}: {text}'


def test_the_unspoiled_input_reaches_the_library(no_library):
    for caller, call in CALLS.items():
        if caller == 'cells':
            assert len(call(good())) == 10      # check_cell_call is the checks alone: it returns the arrays of the library call
        else:
            with pytest.raises(AssertionError, match='the library was loaded'):
                call(good())


def test_region_limits_and_the_limits_themselves():
    from ppopt_amd import region_merge
    assert (_pairs.MAX_DIM, _pairs.MAX_ROWS) == (16, 256) == (region_merge.MAX_DIM, region_merge.MAX_ROWS) and bp.MAX_DIM == 16 == reduce_module.MAX_DIM
    big = CriticalRegion(None, None, None, None, numpy.zeros((257, 2)), numpy.zeros((257, 1)), [])
    small = CriticalRegion(None, None, None, None, numpy.zeros((256, 2)), numpy.zeros((256, 1)), [])
    _pairs.check_region_limits('x', [small, small], 2)
    with pytest.raises(ValueError) as err:
        _pairs.check_region_limits('compare', [small, big], 2, 'of the other solution')
    assert str(err.value) == 'compare: region 1 of the other solution has more than 256 rows'
    with pytest.raises(ValueError) as err:
        _pairs.check_region_limits('remove_overlaps', [small, small, big], 2)
    assert str(err.value) == 'remove_overlaps: region 2 has more than 256 rows'
    with pytest.raises(ValueError) as err:
        _pairs.check_region_limits('transition_graph', [big], 17)
    assert str(err.value) == 'transition_graph: n_theta = 17 > 16'


# ---- 2. the sweep core -------------------------------------------------------------------------------------------------------------------------
def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype == numpy.int64 and numpy.array_equal(g, w)


@pytest.mark.parametrize('R,n_t', [(1, 1), (65, 2), (257, 16)])
def test_the_sweep_core_on_dyadic_boxes(R, n_t):
    """every difference of two bounds is exact on these boxes (multiples of 2^-10 below 8), so the core and the reference decide alike"""
    a, b = ref.dyadic_boxes(R, n_t, 3 * n_t + 1), ref.dyadic_boxes(R, n_t, 3 * n_t + 2)
    use, idx = numpy.ones(R, dtype=bool), numpy.arange(R)
    family = numpy.arange(2 * R) < R
    total = 0
    for margin in (TOL, -TOL):
        one = _pairs.sweep_boxes(a[:, 0], a[:, 1], idx, None, margin)
        _same(one, ref.all_pairs(a, use, margin=margin))
        two = _pairs.sweep_boxes(numpy.concatenate([a[:, 0], b[:, 0]]), numpy.concatenate([a[:, 1], b[:, 1]]), numpy.concatenate([idx, idx]), family, margin)
        _same(two, ref.all_pairs(a, use, b, use, margin))
        for passes in (False, True):      # no NaN difference on these boxes: the flag changes nothing
            _same(_pairs.sweep_boxes(a[:, 0], a[:, 1], idx, None, margin, nan_passes=passes), one)
        total += len(one[0]) + len(two[0])
    assert total > 0 or R == 1


def test_the_nan_difference_flag():
    """the seven boxes of test_box_pairs_cpu's corner cases with their NaN coordinates opened: box 5 has lower = upper = +inf in
    coordinate 1, so its difference with the whole space (1) and with itself is inf - inf there"""
    whole = [[-INF, -INF], [INF, INF]]
    fam = numpy.array([[[0.0, 0.0], [1.0, 1.0]], whole, [[2.0, -INF], [INF, 0.5]], [[0.5, 0.5], [NAN, 0.75]], [[NAN, 3.0], [0.25, 4.0]],
                       [[0.5, INF], [0.75, INF]], [[0.5, 0.25], [NAN, 0.75]]])
    opened, use = _pairs.NAN_RULES['coordinate'][0](fam, numpy.ones(7, dtype=bool))
    assert not numpy.isnan(opened).any() and numpy.isnan(fam).any() and use.all()
    idx = numpy.arange(7)
    args = (numpy.concatenate([opened[:, 0]] * 2), numpy.concatenate([opened[:, 1]] * 2), numpy.concatenate([idx, idx]), numpy.arange(14) < 7, -TOL)
    off = _pairs.sweep_boxes(*args)
    _same(off, ref.all_pairs(opened, use, opened, use, -TOL))
    on = _pairs.sweep_boxes(*args, nan_passes=True)
    pairs = lambda p: set(zip(p[0].tolist(), p[1].tolist()))
    assert pairs(on) - pairs(off) == {(1, 5), (5, 1), (5, 5)} and pairs(off) <= pairs(on)
    _same(on, transition.image_box_pairs(fam, fam, use, TOL))


# ---- 3. the keys of stats with the host sweep and no screen ------------------------------------------------------------------------------------
@pytest.fixture
def fake_library(monkeypatch):
    """fixed answers for unit squares: all feasible at (0.5, 0.5) with the box [0, 1]^2, every pair with radius 0"""
    calls = []

    def merge_regions(off, ef, device=0):
        calls.append('merge_regions')
        R = len(off) - 1
        return numpy.full((R, 2), 0.5), numpy.tile(good()['box'][:1], (R, 1, 1)), numpy.zeros(R, dtype=numpy.int32), {'lps': R, 'pivots': 3 * R, 'capped': 0, 'ms': 0.0}

    def transition_boxes(off, ef, Phi, phi, xs, device=0):
        calls.append('transition_boxes')
        return good()['box'], numpy.zeros(2, dtype=numpy.int32), {'lps': 8, 'pivots': 16, 'ms': 0.0}

    def pairs_of(name, n, more):
        calls.append(name)
        return (numpy.zeros(n),) + more + ({'lps': n, 'pivots': n, 'capped': 0, 'ms': 0.0, 'pairs': n, 'meets': 0, 'constant_rows': 0, 'wide': 0},)

    monkeypatch.setattr(_lib, 'merge_regions', merge_regions)
    monkeypatch.setattr(_lib, 'transition_boxes', transition_boxes)
    monkeypatch.setattr(_lib, 'overlap_pairs', lambda off, ef, xs, pa, pb, *a: pairs_of('overlap_pairs', len(pa), (numpy.full(len(pa), NAN),) * 2 + (numpy.zeros(len(pa), dtype=numpy.int32),)))
    monkeypatch.setattr(_lib, 'transition_pairs', lambda off, ef, Phi, phi, xs, pa, pb, *a: pairs_of('transition_pairs', len(pa), (numpy.zeros(len(pa), dtype=numpy.int32), numpy.zeros((len(pa), 2)))))
    monkeypatch.setattr(_lib, 'law_gap_pairs', lambda off, ef, laws, xs, pa, pb, *a, **k: pairs_of(
        'law_gap_pairs', len(pa), (numpy.full(len(pa), NAN), numpy.full(len(pa), -1, dtype=numpy.int32), numpy.zeros((len(pa), 2)), None, numpy.zeros(len(pa), dtype=numpy.int32))))
    return calls


def test_stats_keys_with_the_host_sweep_and_no_screen(fake_library):
    a = good()
    part = overlap.partition_by_value(a['off'], a['ef'], a['g'], a['h'], 2)
    assert set(part.stats) == {'regions_before', 'candidate_pairs', 'rounds', 'work_items', 'max_item_rows', 'lps', 'pivots', 'wide', 'device_ms',
                               'regions_after', 'wall_ms'}
    assert part.stats['candidate_pairs'] == 1 and fake_library == ['merge_regions', 'overlap_pairs']
    del fake_library[:]
    res = transition.transition_pairs(a['off'], a['ef'], a['Phi'], a['phi'], 2)
    keys = {'box_ms', 'pair_ms', 'sweep_ms', 'candidates', 'lps', 'pivots', 'capped', 'edges', 'box_lps', 'box_pivots'}
    assert set(res['stats']) == keys and res['stats']['candidates'] == 4 and res['stats']['sweep_ms'] > 0.0 and 'screen_box' not in res
    assert fake_library == ['merge_regions', 'transition_boxes', 'transition_pairs']
    del fake_library[:]
    given = transition.transition_pairs(a['off'], a['ef'], a['Phi'], a['phi'], 2, pairs=([1], [0]))
    assert set(given['stats']) == keys and given['stats']['sweep_ms'] == 0.0 and fake_library == ['merge_regions', 'transition_pairs']
    del fake_library[:]
    regs = [CriticalRegion(numpy.zeros((1, 2)), numpy.zeros((1, 1)), numpy.zeros((0, 2)), numpy.zeros((0, 1)), SQUARE[:, 1:].copy(), SQUARE[:, :1].copy(), [k])
            for k in range(2)]
    sol = Solution(None, regs, is_overlapping=False)
    gap = compare.compare_solutions(sol, sol)
    assert set(gap.stats) == {'pairs', 'meets', 'constant_rows', 'lps', 'pivots', 'wide', 'pair_ms', 'device_ms', 'candidates', 'box_pairs', 'sweep_ms', 'wall_ms'}
    assert gap.stats['candidates'] == 4 == gap.stats['box_pairs'] and fake_library == ['merge_regions', 'law_gap_pairs']
