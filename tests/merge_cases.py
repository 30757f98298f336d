"""Random partitions for the merge tests that reach the shapes where the merge kernels can go wrong: several law groups,
holes, thin cells, overlapping sources, wide parameter spaces and regions of more than 64 and more than 128 rows.

A case: a random polytope of 3 n + 4 unit rows with offsets in [0.8, 1.2] (plus ``pad`` rows tangent to the ball of radius 0.7, all of
them facets), cut by ``cuts`` random hyperplanes with offsets in [-0.3, 0.3]; every sign pattern's cell, made irredundant with one LP
per row; a cell goes when its Chebyshev radius is below ``thin`` and, with probability ``drop``, anyway (holes); each kept cell gets
one of ``nlaws`` random laws; ``grown`` of the regions are replaced by themselves with f increased by 0.01 to 0.1 (an overlapping
source).  ``sliver`` > 0 makes the last cut a copy of the first one shifted by that much, so that cells of that width exist.

    CASES            name -> parameters (with the seed)
    build(name)      -> Solution (cached)
    reference(name)  -> (merged Solution of region_merge_reference.merge_reference, info), computed once and shared

For every committed seed the reference meets no LP value within its KNIFE of a threshold and merges at least once
(tests/test_merge_exact_cpu.py checks both), so the device tests need no exemption.
"""
import itertools

import numpy
from scipy.optimize import linprog

import region_merge_reference as ref
from ppopt_amd.critical_region import CriticalRegion
from ppopt_amd.solution import Solution

TOL = 1e-8


class _Prog:
    def __init__(self, n_t):
        self._nt = n_t

    def num_t(self):
        return self._nt


def _radius(E, f):
    n = E.shape[1]
    r = linprog(numpy.append(numpy.zeros(n), -1.0), A_ub=numpy.column_stack([E, numpy.linalg.norm(E, axis=1)]), b_ub=f,
                bounds=[(None, None)] * n + [(0, None)], method='highs')
    return -r.fun if r.status == 0 else -1.0


def _facets(E, f):
    """indices of the rows of {E x <= f} that are facets: the row's maximum with itself relaxed by 1 exceeds its offset"""
    n = E.shape[1]
    keep = []
    for i in range(len(E)):
        b = f.copy()
        b[i] += 1.0
        lp = linprog(-E[i], A_ub=E, b_ub=b, bounds=[(None, None)] * n, method='highs')
        if lp.status != 0 or -lp.fun > f[i] + 1e-9:
            keep.append(i)
    return keep


def random_partition(seed, n, cuts, nlaws=1, drop=0.0, thin=1e-3, grown=0, pad=0, sliver=0.0):
    rng = numpy.random.default_rng(seed)
    m = 3 * n + 4
    E0 = rng.normal(size=(m + pad, n))
    E0 /= numpy.linalg.norm(E0, axis=1, keepdims=True)
    if pad and n == 2:   # a polygon's sides at jittered even angles, so that no two of them are nearly parallel
        ang = 2.0 * numpy.pi * (numpy.arange(pad) + rng.uniform(0.0, 0.5, size=pad)) / pad
        E0[m:] = numpy.column_stack([numpy.cos(ang), numpy.sin(ang)])
    f0 = numpy.concatenate([rng.uniform(0.8, 1.2, size=m), numpy.full(pad, 0.7)])
    H = rng.normal(size=(cuts, n))
    H /= numpy.linalg.norm(H, axis=1, keepdims=True)
    h = rng.uniform(-0.3, 0.3, size=cuts)
    if sliver > 0.0:
        H[-1], h[-1] = H[0], h[0] + sliver
    laws = [(rng.normal(size=(2, n)), rng.normal(size=(2, 1))) for _ in range(nlaws)]
    cells = []
    for signs in itertools.product((1.0, -1.0), repeat=cuts):
        s = numpy.asarray(signs)
        E = numpy.vstack([E0, s[:, None] * H])
        f = numpy.concatenate([f0, s * h])
        if _radius(E, f) < thin or rng.uniform() < drop:
            continue
        keep = _facets(E, f)
        cells.append((E[keep], f[keep]))
    law_of = rng.integers(0, nlaws, size=len(cells))
    grow = set(rng.choice(len(cells), size=min(grown, len(cells)), replace=False).tolist()) if grown else set()
    regs = []
    for k, (E, f) in enumerate(cells):
        if k in grow:
            f = f + rng.uniform(0.01, 0.1)
        A, b = laws[law_of[k]]
        regs.append(CriticalRegion(A.copy(), b.copy(), numpy.zeros((0, n)), numpy.zeros((0, 1)), E, f.reshape(-1, 1), []))
    sol = Solution(_Prog(n), regs, point_location_tolerance=1e-5)
    sol.is_complete = False
    return sol


# the smallest shapes that still reach several rounds, several law groups, holes, thin cells and overlaps; two wide cases; one case
# whose regions pass 64 and 128 rows (a polygon of 236 sides: mask words 1 to 3 and the 64-rows-at-a-time loop of k_merge_pairs)
CASES = {
    'n2_c3_one_law': dict(seed=1, n=2, cuts=3),
    'n2_c5_three_laws_holes': dict(seed=2, n=2, cuts=5, nlaws=3, drop=0.2),
    'n2_c6_slivers': dict(seed=3, n=2, cuts=6, nlaws=2, thin=3e-8, sliver=2e-6),
    'n2_c4_grown': dict(seed=4, n=2, cuts=4, nlaws=2, grown=3),
    'n3_c4_two_laws': dict(seed=5, n=3, cuts=4, nlaws=2),
    'n3_c5_holes_slivers': dict(seed=6, n=3, cuts=5, nlaws=2, drop=0.2, thin=3e-8, sliver=1e-6),
    'n3_c4_grown_holes': dict(seed=7, n=3, cuts=4, nlaws=1, drop=0.2, grown=3),
    'n4_c3_one_law': dict(seed=8, n=4, cuts=3),
    'n4_c5_three_laws_holes_thin': dict(seed=9, n=4, cuts=5, nlaws=3, drop=0.2, thin=3e-8),
    'n4_c4_grown': dict(seed=10, n=4, cuts=4, nlaws=2, grown=3),
    'n8_c4_wide': dict(seed=11, n=8, cuts=4, nlaws=2),
    'n16_c3_wide': dict(seed=12, n=16, cuts=3, nlaws=1, drop=0.2),
    'n2_c3_padded_236_rows': dict(seed=13, n=2, cuts=3, pad=236),
}

_BUILT, _REFERENCE = {}, {}


def build(name):
    if name not in _BUILT:
        _BUILT[name] = random_partition(**CASES[name])
    return _BUILT[name]


def reference(name):
    """(merged, info) of the CPU reference on build(name); shared among the tests, which leave it unchanged"""
    if name not in _REFERENCE:
        _REFERENCE[name] = ref.merge_reference(build(name), None, TOL, TOL)
    return _REFERENCE[name]


def rows_of(region):
    return numpy.asarray(region.E, float), numpy.asarray(region.f, float).reshape(-1)
