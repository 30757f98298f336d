"""Independent CPU builder of point-location search trees: lo / hi of every (region, plane) pair by
scipy.optimize.linprog (HiGHS) on the expanded polytopes, then the classification, split rule, stopping rule and node order of
mpc_tree_build.  Small cases only: one LP per pair and side."""
import numpy
from scipy.optimize import linprog

ALLOW = 1e-9
KNIFE = 1e-9   # a pair whose lo / hi lies this close to -band / +band may be classified either way

# HiGHS's default feasibility tolerances (1e-7) let a vertex between nearly parallel rows be off by 3e-8 (merge_exact_reference.py); the
# rounding allowance check_tree has to resolve is 1e-9, so the LPs run at 1e-10
_HIGHS = {'primal_feasibility_tolerance': 1e-10, 'dual_feasibility_tolerance': 1e-10}


class Classification(tuple):
    """(plus, minus, lo, hi, allow) of classify(); xopt [R, H, 2, n] holds the optimisers of lo / hi (nan where there is none)"""
    xopt = None


def expanded(ef, row_off, r, tol):
    """(A, b) of P^_r = {E_i theta <= f_i + tol max(1, |E_i|)} (zero rows dropped; None if a zero row empties it)."""
    rows = ef[row_off[r]:row_off[r + 1]]
    E, f = rows[:, 1:], rows[:, 0]
    nrm = numpy.linalg.norm(E, axis=1)
    rhs = f + tol * numpy.maximum(1.0, nrm)
    if numpy.any((nrm == 0) & (rhs < 0)):
        return None
    keep = nrm > 0
    return E[keep], rhs[keep]


def _min(c, A, b, n):
    """(min c.x over A x <= b, x*) with -inf for unbounded and None for empty."""
    if len(A) == 0:
        return (-numpy.inf if numpy.any(c != 0) else 0.0), numpy.zeros(n)
    # at 1e-10 HiGHS gives up on about one LP in 3000 of the random sets ("model_status is Unknown; primal_status is Infeasible") although
    # the same LP on unit rows, or on the raw rows where the unit rows fail, or by its interior-point method, ends optimal with the same
    # value to 1e-14: the same tolerances on another statement of the same LP, never looser ones
    nrm = numpy.linalg.norm(A, axis=1)
    for rows, rhs, method in ((A, b, 'highs'), (A / nrm[:, None], b / nrm, 'highs'), (A / nrm[:, None], b / nrm, 'highs-ipm')):
        res = linprog(c, A_ub=rows, b_ub=rhs, bounds=[(None, None)] * n, method=method, options=_HIGHS)
        if res.status in (0, 2, 3):
            break
    if res.status == 3:
        return -numpy.inf, None
    if res.status == 2:
        return None, None
    assert res.status == 0, res.message
    return float(res.fun), res.x


def classify(ef, row_off, planes, tol, band):
    """plus, minus [R, H] bool; lo, hi [R, H] (nan for an empty region); allowances [R, H, 2] of lo / hi."""
    R, H = len(row_off) - 1, len(planes)
    n = planes.shape[1] - 1
    plus, minus = numpy.zeros((R, H), bool), numpy.zeros((R, H), bool)
    lo, hi = numpy.full((R, H), numpy.nan), numpy.full((R, H), numpy.nan)
    allow = numpy.zeros((R, H, 2))
    xopt = numpy.full((R, H, 2, n), numpy.nan)
    for r in range(R):
        P = expanded(ef, row_off, r, tol)
        if P is None:
            continue
        A, b = P
        for h in range(H):
            nv, o = planes[h, :n], planes[h, n]
            vlo, xlo = _min(nv, A, b, n)
            if vlo is None:   # empty: straddles everything
                break
            vhi, xhi = _min(-nv, A, b, n)
            lo[r, h] = vlo - o
            hi[r, h] = -vhi - o
            allow[r, h, 0] = ALLOW * (1 + abs(o) + (numpy.abs(xlo).sum() if xlo is not None else 0))
            allow[r, h, 1] = ALLOW * (1 + abs(o) + (numpy.abs(xhi).sum() if xhi is not None else 0))
            if xlo is not None:
                xopt[r, h, 0] = xlo
            if xhi is not None:
                xopt[r, h, 1] = xhi
            plus[r, h] = lo[r, h] >= -band
            minus[r, h] = hi[r, h] <= band
    out = Classification((plus, minus, lo, hi, allow))
    out.xopt = xopt
    return out


def reband(cls, band):
    """the classification at another band: lo / hi do not depend on it, so no LP is solved again"""
    _, _, lo, hi, allow = cls
    with numpy.errstate(invalid='ignore'):
        out = Classification((lo >= -band, hi <= band, lo, hi, allow))
    out.xopt = cls.xopt
    return out


def knife_pairs(cls, band):
    """(pairs whose lo / hi lies within KNIFE of -band / +band, the smallest such distance over all pairs)"""
    _, _, lo, hi, _ = cls
    d = numpy.concatenate([numpy.abs(lo + band).ravel(), numpy.abs(hi - band).ravel()])
    d = d[numpy.isfinite(d)]
    return int(numpy.sum(d <= KNIFE)), (float(d.min()) if len(d) else numpy.inf)


def build(ef, row_off, planes, cand_start, cand_plane, tol, band, leaf_size=1, max_depth=48, cls=None):
    """The tree mpc_tree_build builds from exact classifications: dict of the SearchTree arrays, plus 'tau_raw' (tau without the
    rounding allowance) and the classification used."""
    R, H = len(row_off) - 1, len(planes)
    cls = cls if cls is not None else classify(ef, row_off, planes, tol, band)
    plus, minus, lo, hi, allow = cls
    po, mo = plus & ~minus, minus & ~plus
    owner = None
    if cand_start is not None:
        owner = [set(int(h) for h in cand_plane[cand_start[r]:cand_start[r + 1]]) for r in range(R)]
    nodes = [{'plane': -1, 'child': [-1, -1], 'tau': [0.0, 0.0], 'raw': [0.0, 0.0], 'depth': 0, 'list': list(range(R))}]
    level = [0]
    while level and H > 0:
        work = [k for k in level if len(nodes[k]['list']) > leaf_size and nodes[k]['depth'] < max_depth]
        if not work:
            break
        nxt = []
        for k in work:
            nd = nodes[k]
            lst = numpy.array(nd['list'], dtype=numpy.int64)
            size = len(lst)
            cands = sorted(set().union(*(owner[j] for j in lst))) if owner is not None else range(H)
            best = None
            for h in cands:
                np_, nm = int(po[lst, h].sum()), int(mo[lst, h].sum())
                n0 = size - np_ - nm
                key = (max(np_, nm) + n0, n0, h)
                if best is None or key < best:
                    best = key
            if best is None or best[0] >= size:
                continue
            h = best[2]
            nd['plane'] = h
            cp = [int(j) for j in lst if not mo[j, h]]
            cm = [int(j) for j in lst if not po[j, h]]
            for side, sel in ((0, po), (1, mo)):
                t_raw, t = 0.0, 0.0
                for j in lst[sel[lst, h]]:
                    v = -lo[j, h] if side == 0 else hi[j, h]
                    t_raw = max(t_raw, max(0.0, v))
                    t = max(t, max(0.0, v) + allow[j, h, side])
                nd['tau'][side], nd['raw'][side] = t, t_raw
            ip = len(nodes)
            nd['child'] = [ip, ip + 1]
            nd['list'] = []
            for lst_c in (cp, cm):
                nodes.append({'plane': -1, 'child': [-1, -1], 'tau': [0.0, 0.0], 'raw': [0.0, 0.0], 'depth': nd['depth'] + 1, 'list': lst_c})
            nxt += [ip, ip + 1]
        level = nxt
    N = len(nodes)
    off = numpy.zeros(N + 1, dtype=numpy.int64)
    items = []
    for k, nd in enumerate(nodes):
        if nd['plane'] < 0:
            items += nd['list']
        off[k + 1] = len(items)
    return {'planes': numpy.asarray(planes, dtype=float), 'node_plane': numpy.array([nd['plane'] for nd in nodes], dtype=numpy.int32),
            'node_child': numpy.array([nd['child'] for nd in nodes], dtype=numpy.int32).reshape(N, 2),
            'node_tau': numpy.array([nd['tau'] for nd in nodes]).reshape(N, 2), 'tau_raw': numpy.array([nd['raw'] for nd in nodes]).reshape(N, 2),
            'node_off': off, 'items': numpy.array(items, dtype=numpy.int32), 'tol': float(tol), 'band': float(band),
            'classification': cls}


def scan(ef, row_off, xlaw, theta, tol, overlapping=False, inclusive=False, Q=None, c=None, H=None):
    """numpy re-statement of the list scan (k_locate): first containing region, or the lowest objective with ties to the later."""
    found, best = -1, numpy.inf
    for r in range(len(row_off) - 1):
        rows = ef[row_off[r]:row_off[r + 1]]
        if len(rows) == 0:   # k_locate walks rows: a region without rows is never met
            continue
        if inclusive:
            inside = numpy.all(rows[:, 1:] @ theta <= rows[:, 0] + tol)
        else:
            inside = numpy.all(rows[:, 1:] @ theta - rows[:, 0] < tol)
        if not inside:
            continue
        if not overlapping:
            return r
        x = xlaw[r][:, 0] + xlaw[r][:, 1:] @ theta
        g = numpy.zeros_like(x) if c is None else numpy.asarray(c, float).reshape(-1).copy()
        if H is not None:
            g = g + numpy.asarray(H, float).reshape(len(x), -1) @ theta
        if Q is not None:
            g = g + 0.5 * (numpy.asarray(Q, float) @ x)
        obj = float(g @ x)
        if obj <= best:
            best, found = obj, r
    return found


def near_split_points(arrays, ef, row_off, tol, rng, per=4):
    """Points at +-{0.5, 0.99, 1.01} tol (row-norm scaled) from the facets of regions next to split planes."""
    planes, node_plane = arrays['planes'], arrays['node_plane']
    n = planes.shape[1] - 1
    used = set(int(h) for h in node_plane if h >= 0)
    pts = []
    for r in range(len(row_off) - 1):
        rows = ef[row_off[r]:row_off[r + 1]]
        for row in rows:
            nrm = numpy.linalg.norm(row[1:])
            if nrm == 0:
                continue
            u = numpy.concatenate([row[1:], [row[0]]]) / nrm
            hits = [h for h in used if numpy.allclose(numpy.abs(planes[h] @ u), 1.0, atol=1e-9) or numpy.allclose(planes[h], u, atol=1e-9)
                    or numpy.allclose(planes[h], -u, atol=1e-9)]
            if not hits:
                continue
            # a point on the facet: a random point projected onto the row's plane, then pushed along the normal
            for _ in range(per):
                p = rng.normal(size=n) * 0.3 + _centre(rows)
                p = p - (row[1:] @ p - row[0]) / nrm ** 2 * row[1:]
                for k in (0.5, 0.99, 1.01):
                    for sgn in (-1.0, 1.0):
                        pts.append(p + sgn * k * tol * max(1.0, nrm) / nrm * row[1:] / nrm)
    return numpy.array(pts).reshape(-1, n)


def _centre(rows, or_none=False):
    """Chebyshev centre of {E theta <= f} (radius capped at 1e3); the origin, or None with or_none, where there is none"""
    A, b = rows[:, 1:], rows[:, 0]
    n = A.shape[1]
    nrm = numpy.linalg.norm(A, axis=1, keepdims=True)
    res = linprog(numpy.r_[numpy.zeros(n), -1.0], A_ub=numpy.hstack([A, nrm]), b_ub=b, bounds=[(None, None)] * n + [(0, 1e3)],
                  method='highs')
    if or_none:
        return res.x[:n] if res.status == 0 and len(rows) and res.x[n] > 0 else None
    return res.x[:n] if res.status == 0 else numpy.zeros(n)


# ---- the checker of any builder's tree ---------------------------------------------------------------------------------------------------
def _bounds(cls):
    """bound [R, H, 2] of a region that is dropped on side s of a plane: -lo for s = 0 (covered by tau-), hi for s = 1 (tau+); an empty
    expanded polytope (nan) may never be dropped: +inf"""
    _, _, lo, hi, _ = cls
    b = numpy.stack([-lo, hi], axis=2)
    b[numpy.isnan(b)] = numpy.inf
    return b


def _subtree_sets(arrays):
    """(sets, depth, structure): the union of the leaf lists under every node, every node's depth, and what is wrong with the arrays"""
    plane, child, off, items = arrays['node_plane'], numpy.asarray(arrays['node_child']).reshape(-1, 2), arrays['node_off'], arrays['items']
    N = len(plane)
    wrong = []
    if len(off) != N + 1 or off[0] != 0 or numpy.any(numpy.diff(off) < 0) or off[-1] != len(items):
        wrong.append('node_off is not N + 1 non-decreasing offsets over items')
    parents = numpy.zeros(N, dtype=int)
    for k in range(N):
        lst = items[off[k]:off[k + 1]]
        if plane[k] >= 0:
            if len(lst):
                wrong.append(f'inner node {k} has a list')
            if not all(k < c < N for c in child[k]) or child[k][0] == child[k][1]:
                wrong.append(f'node {k}: children {child[k].tolist()} do not come after their parent')
            else:
                parents[child[k]] += 1
        elif numpy.any(numpy.diff(lst) <= 0):
            wrong.append(f'leaf {k}: the list does not ascend')
    if numpy.any(parents[1:] != 1) or parents[0] != 0:
        wrong.append('a node other than the root has not exactly one parent')
    sets, depth = [set()] * N, numpy.zeros(N, dtype=int)
    if not wrong:
        for k in range(N):
            if plane[k] >= 0:
                depth[child[k]] = depth[k] + 1
        for k in reversed(range(N)):
            sets[k] = set(items[off[k]:off[k + 1]].tolist()) if plane[k] < 0 else sets[child[k][0]] | sets[child[k][1]]
    return sets, depth, wrong


def check_tree(arrays, ef, row_off, tol, band, cls, max_depth, leaf_size=1, cand=None):
    """What is wrong with a tree (SearchTree arrays of any builder) by the exact lo / hi of ``cls`` (the tuple of classify()); asserts
    nothing.  A node's set is the union of the leaf lists below it.  side 0 is tau- (node_tau[k, 0], covers the regions absent from the
    "-" subtree with bound -lo), side 1 is tau+ (absent from the "+" subtree, bound hi).  cand: (cand_start, cand_plane) or None for
    every plane a candidate.  The record:
      structure      messages: children after their parent, ascending leaf lists, node_off consistent, the root's set every region
      unsound        (node, side, region, bound, tau) with bound > tau, no margin: the tree loses points of the region
      missing        (leaf, region): the region is absent from a leaf that points of it reach (unsound followed down from the root)
      not_one_sided  (node, side, region, bound) of dropped regions with bound > band + KNIFE
      loose          (node, side, tau, limit) with tau > limit = 2 max (max(0, bound) + allow) + 1e-12 over the tree's own dropped regions
      stopped_early  (leaf, size, plane, key): a leaf of more than leaf_size regions above max_depth although a candidate has key < size
      margin         the smallest tau - bound over the dropped pairs with a finite bound (inf if there is none);  dropped: their count"""
    R = len(row_off) - 1
    plane, child, tau = arrays['node_plane'], numpy.asarray(arrays['node_child']).reshape(-1, 2), numpy.asarray(arrays['node_tau']).reshape(-1, 2)
    allow = cls[4]
    bound = _bounds(cls)
    with numpy.errstate(invalid='ignore'):
        po, mo = (cls[2] >= -band) & ~(cls[3] <= band), (cls[3] <= band) & ~(cls[2] >= -band)
    sets, depth, wrong = _subtree_sets(arrays)
    rec = {'structure': wrong, 'unsound': [], 'missing': [], 'not_one_sided': [], 'loose': [], 'stopped_early': [], 'margin': numpy.inf,
           'dropped': 0}
    if wrong:
        return rec
    N = len(plane)
    if sets[0] != set(range(R)):
        wrong.append(f'the root holds {sorted(sets[0])}, not every region')
    reach = [set() for _ in range(N)]   # regions with points that the descent can bring to the node
    reach[0] = set(range(R))
    for k in range(N):
        h = plane[k]
        if h < 0:
            rec['missing'] += [(k, j) for j in sorted(reach[k] - sets[k])]
            size = len(sets[k])
            if size > leaf_size and depth[k] < max_depth:
                lst = numpy.array(sorted(sets[k]), dtype=numpy.int64)
                if cand is None:
                    cands = range(len(arrays['planes']))
                else:
                    cands = sorted(set(int(q) for j in lst for q in cand[1][cand[0][j]:cand[0][j + 1]]))
                keys = [(max(int(po[lst, q].sum()), int(mo[lst, q].sum())) + size - int(po[lst, q].sum()) - int(mo[lst, q].sum()), q) for q in cands]
                if keys and min(keys)[0] < size:
                    rec['stopped_early'].append((k, size, min(keys)[1], min(keys)[0]))
            continue
        # the "+" child (0) lacks the regions covered by tau+ (side 1), the "-" child (1) those covered by tau- (side 0)
        for side, c in ((1, child[k][0]), (0, child[k][1])):
            t = tau[k, side]
            limit = 0.0
            for j in sorted(sets[k] - sets[c]):
                b = bound[j, h, side]
                rec['dropped'] += 1
                if b > t:
                    rec['unsound'].append((k, side, j, float(b), float(t)))
                elif numpy.isfinite(b):
                    rec['margin'] = min(rec['margin'], float(t - b))
                if b > band + KNIFE:
                    rec['not_one_sided'].append((k, side, j, float(b)))
                limit = max(limit, max(0.0, b) + allow[j, h, side])
            if t > 2.0 * limit + 1e-12:
                rec['loose'].append((k, side, float(t), 2.0 * limit + 1e-12))
            reach[c] |= {j for j in reach[k] if j in sets[c] or bound[j, h, side] > t}
    return rec


def witness_points(arrays, ef, row_off, tol, cls, pull=1e-3):
    """(points [P, n], nodes [P], regions [P], inner nodes with a dropped region): for every (inner node, dropped region) pair the point
    of the expanded region farthest over the node's plane (the reference optimiser of the bound), pulled by ``pull`` of the distance towards
    the region's Chebyshev centre.  Of all the region's points it is the first one a short tau would lose.  Regions without a centre and
    unbounded bounds have none."""
    plane, child = arrays['node_plane'], numpy.asarray(arrays['node_child']).reshape(-1, 2)
    n = arrays['planes'].shape[1] - 1
    sets, _, wrong = _subtree_sets(arrays)
    assert not wrong, wrong
    centres = {}
    pts, nodes, regions, with_dropped = [], [], [], set()
    for k in range(len(plane)):
        h = plane[k]
        if h < 0:
            continue
        for side, c in ((1, child[k][0]), (0, child[k][1])):
            for j in sorted(sets[k] - sets[c]):
                with_dropped.add(k)
                if j not in centres:
                    centres[j] = _centre(ef[row_off[j]:row_off[j + 1]], or_none=True)
                x = cls.xopt[j, h, side]
                if centres[j] is None or not numpy.all(numpy.isfinite(x)):
                    continue
                pts.append(x + pull * (centres[j] - x))
                nodes.append(k)
                regions.append(j)
    return numpy.array(pts).reshape(-1, n), numpy.array(nodes, dtype=int), numpy.array(regions, dtype=int), sorted(with_dropped)
