"""Independent CPU builder of point-location search trees: lo / hi of every (region, plane) pair by
scipy.optimize.linprog (HiGHS) on the expanded polytopes, then the classification, split rule, stopping rule and node order of
mpc_tree_build.  Small cases only: one LP per pair and side."""
import numpy
from scipy.optimize import linprog

ALLOW = 1e-9


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
    res = linprog(c, A_ub=A, b_ub=b, bounds=[(None, None)] * n, method='highs')
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
            plus[r, h] = lo[r, h] >= -band
            minus[r, h] = hi[r, h] <= band
    return plus, minus, lo, hi, allow


def build(ef, row_off, planes, cand_start, cand_plane, tol, band, leaf_size=1, max_depth=48, cls=None):
    """The tree mpc_tree_build builds from exact classifications: dict of the SearchTree arrays, plus 'tau_raw' (tau without the
    rounding allowance) and the classification used."""
    R, H = len(row_off) - 1, len(planes)
    plus, minus, lo, hi, allow = cls if cls is not None else classify(ef, row_off, planes, tol, band)
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
            'classification': (plus, minus, lo, hi, allow)}


def scan(ef, row_off, xlaw, theta, tol, overlapping=False, inclusive=False, Q=None, c=None, H=None):
    """numpy re-statement of the list scan (k_locate): first containing region, or the lowest objective with ties to the later."""
    found, best = -1, numpy.inf
    for r in range(len(row_off) - 1):
        rows = ef[row_off[r]:row_off[r + 1]]
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


def _centre(rows):
    A, b = rows[:, 1:], rows[:, 0]
    n = A.shape[1]
    nrm = numpy.linalg.norm(A, axis=1, keepdims=True)
    res = linprog(numpy.r_[numpy.zeros(n), -1.0], A_ub=numpy.hstack([A, nrm]), b_ub=b, bounds=[(None, None)] * n + [(0, 1e3)],
                  method='highs')
    return res.x[:n] if res.status == 0 else numpy.zeros(n)
