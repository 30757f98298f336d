"""Merging regions with equal control laws into convex unions (Solution.merge_regions).

A deployed explicit controller applies only some rows of x*(theta) (the first input of an MPC law).  Many regions give the same law
for those rows; where two of them form a convex union they can be replaced by it.  The merge is greedy, pairwise and deterministic:

  1. regions are grouped by law on the host: a region joins the first group (in region order) whose first region's law on ``outputs``
     agrees with its own within law_tol (1 + max |[A | b]|) in every entry, else it opens a group;
  2. candidate pairs lie in one group and have bounding boxes that touch within tol;
  3. every candidate pair is tested on the device (csrc/merge.hpp, k_merge_pairs): the envelope rows of both sides and the convexity
     LPs of Bemporad, Fukuda and Torrisi (2001);
  4. pairs are taken in ascending order of (smallest member of P, smallest member of Q) and accepted when neither region is taken yet
     in this round; the union is the envelope without near-duplicate rows; a union of more than 256 rows is not formed (counted);
  5. the next round tests the pairs that involve a region formed in this one; the merge ends with a round that accepts nothing.

The result is pairwise maximal, not the fewest regions (that problem is NP-hard): three regions with a convex union whose pairwise
unions are not convex stay apart.
"""
import time
from dataclasses import dataclass, field
from typing import List, Optional

import numpy

from ._pairs import MAX_DIM, MAX_ROWS, check_region_limits      # the limits are defined there; importers of this module find them here
from .critical_region import CriticalRegion

__all__ = ['MergedRegion', 'merge_regions', 'build_merged_solution', 'unit_rows', 'solution_rows','law_groups', 'dedupe_rows', 'check_source']


@dataclass(eq=False)
class MergedRegion(CriticalRegion):
    """A region of a merged solution: x[outputs] = A theta + b on {E theta <= f}; ``members`` are ascending indices into the source's
    critical_regions whose union it is.  C, d and active_set are empty: a merged region has no multipliers."""
    members: List[int] = field(default_factory=list)


def check_source(source, outputs, tol: float, law_tol: float):
    """(n_theta, outputs as a list) of a solution merge_regions accepts; ValueError otherwise, before anything reaches the device."""
    if source.is_overlapping:
        raise ValueError('merge_regions: the source is overlapping (every mpLP solution is): a point may lie in several regions and '
                         'the answer there is chosen by objective, not by the law alone')
    if source.is_mixed_integer_sol() or any(r.y_fixation is not None for r in source.critical_regions):
        raise ValueError('merge_regions: mixed-integer solutions are not merged')
    n_t = source.theta_dim() if source.program is not None else numpy.asarray(source.critical_regions[0].E).shape[1]
    check_region_limits('merge_regions', (), n_t)
    if not (numpy.isfinite(tol) and tol >= 0.0 and numpy.isfinite(law_tol) and law_tol >= 0.0):
        raise ValueError('merge_regions: tol and law_tol must be finite and >= 0')
    check_region_limits('merge_regions', source.critical_regions, n_t)
    n_x = numpy.asarray(source.critical_regions[0].A).reshape(-1, n_t).shape[0] if source.critical_regions else None
    if outputs is None:
        outputs = list(range(n_x or 0))
    else:
        outputs = [int(o) for o in outputs]
        if not outputs or (n_x is not None and any(not 0 <= o < n_x for o in outputs)):
            raise ValueError(f'merge_regions: outputs must be a non-empty list of row indices of x in 0..{(n_x or 0) - 1}, got {outputs}')
    return n_t, outputs


def unit_rows(E, f, n_t: int):
    """([m, n_t + 1] unit rows [o | n] of {E theta <= f}, empty): zero rows are dropped, and one with f < 0 empties the region."""
    E = numpy.asarray(E, dtype=numpy.float64).reshape(-1, n_t)
    f = numpy.asarray(f, dtype=numpy.float64).reshape(-1)
    nrm = numpy.linalg.norm(E, axis=1)
    keep = nrm > 0.0
    empty = bool(numpy.any(~keep & (f < 0.0)))
    return numpy.hstack([(f[keep] / nrm[keep]).reshape(-1, 1), E[keep] / nrm[keep, None]]), empty


def solution_rows(regions, n_t: int, who: str):
    """(row_off [R + 1] int64, rows [total, n_t + 1], void) of a solution's regions: their unit rows stacked in CSR form and the indices
    of the regions unit_rows finds empty.  ValueError in the name of ``who`` for a region that keeps no row."""
    rows, void = [], []
    for i, r in enumerate(regions):
        u, empty = unit_rows(r.E, r.f, n_t)
        if not len(u):
            raise ValueError(f'{who}: region {i} has no row with a normal (the whole space, or nothing)')
        rows.append(u)
        if empty:
            void.append(i)
    return numpy.concatenate([[0], numpy.cumsum([len(u) for u in rows])]).astype(numpy.int64), numpy.vstack(rows), void


def law_of(region, outputs, n_t: int) -> numpy.ndarray:
    """[len(outputs), n_t + 1] = [A | b] restricted to the rows ``outputs``."""
    A = numpy.asarray(region.A, dtype=numpy.float64).reshape(-1, n_t)
    b = numpy.asarray(region.b, dtype=numpy.float64).reshape(-1, 1)
    return numpy.hstack([A, b])[outputs]


def law_groups(laws: numpy.ndarray, law_tol: float) -> numpy.ndarray:
    """Group index of every law [R, k]: the first group (in order) whose first law agrees within law_tol (1 + max |first|) in every entry."""
    R = len(laws)
    flat = laws.reshape(R, -1)
    group = numpy.full(R, -1, dtype=numpy.int64)
    reps, scale = numpy.empty_like(flat), numpy.empty(R)
    G = 0
    for i in range(R):
        hit = numpy.flatnonzero(numpy.all(numpy.abs(reps[:G] - flat[i]) <= law_tol * scale[:G, None], axis=1))
        if len(hit):
            group[i] = hit[0]
            continue
        group[i], reps[G], scale[G] = G, flat[i], 1.0 + numpy.max(numpy.abs(flat[i]), initial=0.0)
        G += 1
    return group


def boxes_touch(box_p: numpy.ndarray, box_q: numpy.ndarray, tol: float) -> numpy.ndarray:
    """box [.., 2, n_t] (lower, upper): do the boxes touch within tol max(1, |bound|) in every coordinate?"""
    lo_p, hi_p, lo_q, hi_q = box_p[..., 0, :], box_p[..., 1, :], box_q[..., 0, :], box_q[..., 1, :]
    with numpy.errstate(invalid='ignore'):
        a = lo_p <= hi_q + tol * numpy.maximum(1.0, numpy.abs(hi_q))
        b = lo_q <= hi_p + tol * numpy.maximum(1.0, numpy.abs(hi_p))
    return numpy.all(a & b, axis=-1)


def mask_rows(words: numpy.ndarray, m: int) -> numpy.ndarray:
    """Indices of the set bits 0..m-1 of a row mask [MERGE_WORDS] uint64."""
    bits = numpy.unpackbits(numpy.ascontiguousarray(words, dtype='<u8').view(numpy.uint8), bitorder='little')
    return numpy.flatnonzero(bits[:m])


def dedupe_rows(rows: numpy.ndarray, tol: float) -> numpy.ndarray:
    """Unit rows [o | n] in order without near-duplicates: a row goes when an earlier kept row has every |n_i - n_k| <= tol and
    |o - o_k| <= tol max(1, |o|)."""
    kept = []
    for r in rows:
        dup = False
        for k in kept:
            if numpy.max(numpy.abs(r[1:] - k[1:])) <= tol and abs(r[0] - k[0]) <= tol * max(1.0, abs(r[0])):
                dup = True
                break
        if not dup:
            kept.append(r)
    return numpy.asarray(kept).reshape(-1, rows.shape[1])


def build_merged_solution(source, members, rows, outputs, stats: Optional[dict] = None):
    """The merged Solution from ``members`` (ascending source indices per result region) and ``rows`` (per result region [m, n_t + 1]
    unit rows [o | n], or None for a region of one member, whose E, f are copied unchanged).  Host only: no device is touched."""
    from .solution import Solution
    regs = source.critical_regions
    n_t = source.theta_dim() if source.program is not None else numpy.asarray(regs[0].E).shape[1]
    outputs = [int(o) for o in outputs]
    order = sorted(range(len(members)), key=lambda k: min(members[k]))
    out = []
    for k in order:
        mem = sorted(int(i) for i in members[k])
        first = regs[mem[0]]
        A = numpy.asarray(first.A, dtype=numpy.float64).reshape(-1, n_t)[outputs].copy()
        b = numpy.asarray(first.b, dtype=numpy.float64).reshape(-1, 1)[outputs].copy()
        if rows[k] is None:
            if len(mem) != 1:
                raise ValueError('build_merged_solution: rows may be None only for a region of one member')
            E, f = numpy.array(first.E, dtype=numpy.float64, copy=True), numpy.array(first.f, dtype=numpy.float64, copy=True)
        else:
            rk = numpy.asarray(rows[k], dtype=numpy.float64).reshape(-1, n_t + 1)
            E, f = rk[:, 1:].copy(), rk[:, :1].copy()
        out.append(MergedRegion(A, b, numpy.zeros((0, n_t)), numpy.zeros((0, 1)), E, f, [], members=mem))
    covered = sorted(i for m in members for i in m)
    if covered != list(range(len(regs))):
        raise ValueError('build_merged_solution: the member lists must partition the source regions')
    sol = Solution(source.program, out, is_overlapping=False, point_location_tolerance=source.point_location_tolerance)
    sol.is_complete = source.is_complete
    sol.merge_info = {'source': source, 'outputs': outputs, 'members': [r.members for r in out], 'stats': dict(stats or {})}
    return sol


def merge_regions(source, outputs=None, tol: float = 1e-8, law_tol: float = 1e-8, device: int = 0):
    """Solution.merge_regions (the module docstring).  Returns a new Solution of MergedRegion; the source is not modified."""
    from . import _lib
    t0 = time.perf_counter()
    n_t, outputs = check_source(source, outputs, tol, law_tol)
    regs = source.critical_regions
    R = len(regs)
    groups = law_groups(numpy.asarray([law_of(r, outputs, n_t) for r in regs]).reshape(R, len(outputs), n_t + 1), law_tol) if R else \
        numpy.zeros(0, dtype=numpy.int64)
    stats = {'regions_before': R, 'law_groups': int(groups.max() + 1) if R else 0, 'rounds': 0, 'pairs': 0, 'box_pairs': 0,
             'box_lps': 0, 'lps': 0, 'pivots': 0, 'capped': 0, 'too_many_rows': 0, 'device_ms': 0.0}
    # the current regions, by id (ids of merged regions follow the source's)
    members: List[List[int]] = [[i] for i in range(R)]
    rows, key, group, fresh = [], list(range(R)), list(groups), []
    for i, r in enumerate(regs):
        u, empty = unit_rows(r.E, r.f, n_t)
        rows.append(u)
        if not empty and len(u):      # an empty region, and one without rows (the whole space), never merge
            fresh.append(i)
    alive = set(range(R))
    xs = numpy.zeros((R, n_t))
    box = numpy.zeros((R, 2, n_t))
    usable = numpy.zeros(R, dtype=bool)
    while fresh:
        # feasible points and boxes of the new regions: one launch
        off = numpy.concatenate([[0], numpy.cumsum([len(rows[i]) for i in fresh])]).astype(numpy.int64)
        x_n, b_n, st_n, s = _lib.merge_regions(off, numpy.vstack([rows[i] for i in fresh]), device)
        stats['box_lps'] += s['lps']
        stats['device_ms'] += s['ms']
        need = max(fresh) + 1
        if need > len(xs):
            xs = numpy.vstack([xs, numpy.zeros((need - len(xs), n_t))])
            box = numpy.concatenate([box, numpy.zeros((need - len(box), 2, n_t))])
            usable = numpy.concatenate([usable, numpy.zeros(need - len(usable), dtype=bool)])
        fr = numpy.asarray(fresh)
        xs[fr], box[fr], usable[fr] = x_n, b_n, st_n == 0
        # candidate pairs: a new region and any live region of its group, boxes touching
        by_group = {}
        for i in sorted(alive):
            if usable[i]:
                by_group.setdefault(group[i], []).append(i)
        cand = set()
        for i in fresh:
            if not usable[i]:
                continue
            others = numpy.asarray([j for j in by_group.get(group[i], []) if j != i], dtype=numpy.int64)
            if not len(others):
                continue
            hit = others[boxes_touch(box[i][None], box[others], tol)]
            for j in hit.tolist():
                cand.add((i, j) if key[i] < key[j] else (j, i))
        if not cand:
            break
        pairs = sorted(cand, key=lambda pq: (key[pq[0]], key[pq[1]]))
        stats['rounds'] += 1
        involved = sorted({i for pq in pairs for i in pq})
        local = {g: k for k, g in enumerate(involved)}
        off = numpy.concatenate([[0], numpy.cumsum([len(rows[i]) for i in involved])]).astype(numpy.int64)
        inv = numpy.asarray(involved)
        env_a, env_b, verdict, _, s = _lib.merge_pairs(off, numpy.vstack([rows[i] for i in involved]), xs[inv], box[inv],
                                                       [local[p] for p, _ in pairs], [local[q] for _, q in pairs], tol, device)
        for k in ('pairs', 'box_pairs', 'lps', 'pivots', 'capped'):
            stats[k] += s[k]
        stats['device_ms'] += s['ms']
        taken, fresh = set(), []
        for k, (p, q) in enumerate(pairs):
            if not verdict[k] or p in taken or q in taken:
                continue
            env = numpy.vstack([rows[p][mask_rows(env_a[k], len(rows[p]))], rows[q][mask_rows(env_b[k], len(rows[q]))]])
            u = dedupe_rows(env, tol)
            if len(u) > MAX_ROWS:
                stats['too_many_rows'] += 1
                continue
            taken.update((p, q))
            members.append(sorted(members[p] + members[q]))
            rows.append(u)
            key.append(min(key[p], key[q]))
            group.append(group[p])
            alive.add(len(members) - 1)
            fresh.append(len(members) - 1)
        alive -= taken
    final = sorted(alive, key=lambda i: key[i])
    stats['regions_after'] = len(final)
    stats['wall_ms'] = (time.perf_counter() - t0) * 1e3
    return build_merged_solution(source, [members[i] for i in final], [rows[i] if len(members[i]) > 1 else None for i in final], outputs,
                                 stats)
