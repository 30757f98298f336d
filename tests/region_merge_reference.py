"""An independent CPU statement of Solution.merge_regions: numpy and scipy.optimize.linprog (HiGHS), the same rules and
order, and no package code except build_merged_solution, which only assembles the result.

    merge_reference(solution, outputs, tol, law_tol) -> (merged Solution, info)

info['knife'] counts the pairs tested whose outcome hangs on an LP value within KNIFE of its threshold (a row's max minus its offset
against tol max(1, |o|), or t* against tol): there a device result may differ by rounding, and the tests exempt such cases.
info['tested'] lists every candidate pair in the order tested: (rows of P, rows of Q, valid rows of P, valid rows of Q, convex).
"""
import numpy
from scipy.optimize import linprog

from ppopt_amd.region_merge import build_merged_solution

KNIFE = 1e-9
MAX_ROWS = 256


def _unit(E, f, n_t):
    E = numpy.asarray(E, float).reshape(-1, n_t)
    f = numpy.asarray(f, float).reshape(-1)
    n = numpy.linalg.norm(E, axis=1)
    k = n > 0
    return numpy.column_stack([f[k] / n[k], E[k] / n[k, None]]), bool(numpy.any(~k & (f < 0)))


def _lp_max(c, A, b):
    """max c.x s.t. A x <= b: (value or +inf when unbounded, None when infeasible)"""
    r = linprog(-numpy.asarray(c, float), A_ub=A, b_ub=b, bounds=[(None, None)] * len(c), method='highs')
    if r.status == 3:
        return numpy.inf
    if r.status != 0:
        return None
    return -r.fun


def _box(rows, n_t):
    A, b = rows[:, 1:], rows[:, 0]
    if _lp_max(numpy.zeros(n_t), A, b) is None:
        return None
    lo, hi = numpy.empty(n_t), numpy.empty(n_t)
    for t in range(n_t):
        e = numpy.zeros(n_t)
        e[t] = 1.0
        hi[t] = _lp_max(e, A, b)
        lo[t] = -_lp_max(-e, A, b)
    return lo, hi


def _touch(bp, bq, tol):
    (lp, hp), (lq, hq) = bp, bq
    with numpy.errstate(invalid='ignore'):
        return bool(numpy.all(lp <= hq + tol * numpy.maximum(1.0, numpy.abs(hq))) and numpy.all(lq <= hp + tol * numpy.maximum(1.0, numpy.abs(hp))))


def _valid(rows_y, rows_x, tol, knife):
    """bit per row of Y: max over X of (n.theta - o) <= tol max(1, |o|)"""
    out = numpy.zeros(len(rows_y), dtype=bool)
    for r, row in enumerate(rows_y):
        v = _lp_max(row[1:], rows_x[:, 1:], rows_x[:, 0])
        thr = tol * max(1.0, abs(row[0]))
        out[r] = v is not None and v - row[0] <= thr
        if v is not None and numpy.isfinite(v) and abs(v - row[0] - thr) <= KNIFE:
            knife[0] += 1
    return out


def _pair_test(rp, rq, n_t, tol, knife):
    """(convex, valid rows of P, valid rows of Q)"""
    va, vb = _valid(rp, rq, tol, knife), _valid(rq, rp, tol, knife)
    env = numpy.vstack([rp[va], rq[vb]])
    A_env = numpy.column_stack([env[:, 1:], numpy.zeros(len(env))])
    b_env = env[:, 0] + tol * numpy.maximum(1.0, numpy.abs(env[:, 0]))
    c = numpy.zeros(n_t + 1)
    c[n_t] = 1.0
    for i in numpy.flatnonzero(~va):
        for j in numpy.flatnonzero(~vb):
            A = numpy.vstack([A_env, numpy.append(-rp[i, 1:], 1.0), numpy.append(-rq[j, 1:], 1.0)])
            b = numpy.concatenate([b_env, [-rp[i, 0], -rq[j, 0]]])
            t = _lp_max(c, A, b)
            t = numpy.inf if t is None else t
            if numpy.isfinite(t) and abs(t - tol) <= KNIFE:
                knife[0] += 1
            if not t <= tol:
                return False, va, vb
    return True, va, vb


def _dedupe(rows, tol):
    kept = []
    for r in rows:
        if not any(numpy.max(numpy.abs(r[1:] - k[1:])) <= tol and abs(r[0] - k[0]) <= tol * max(1.0, abs(r[0])) for k in kept):
            kept.append(r)
    return numpy.asarray(kept).reshape(-1, rows.shape[1])


def merge_reference(solution, outputs=None, tol=1e-8, law_tol=1e-8):
    regs = solution.critical_regions
    n_t = numpy.asarray(regs[0].E).shape[1]
    n_x = numpy.asarray(regs[0].A).reshape(-1, n_t).shape[0]
    outputs = list(range(n_x)) if outputs is None else [int(o) for o in outputs]
    R = len(regs)
    # groups: the first group whose first law agrees within law_tol (1 + max |first|)
    group, reps = [], []
    for r in regs:
        law = numpy.column_stack([numpy.asarray(r.A, float).reshape(-1, n_t), numpy.asarray(r.b, float).reshape(-1, 1)])[outputs].ravel()
        g = next((k for k, rep in enumerate(reps) if numpy.all(numpy.abs(rep - law) <= law_tol * (1.0 + numpy.max(numpy.abs(rep))))), None)
        if g is None:
            g = len(reps)
            reps.append(law)
        group.append(g)
    members = [[i] for i in range(R)]
    rows, boxes, fresh = [], [], []
    for i, r in enumerate(regs):
        u, empty = _unit(r.E, r.f, n_t)
        rows.append(u)
        boxes.append(None)
        if not empty and len(u):
            fresh.append(i)
    key = list(range(R))
    alive = set(range(R))
    knife = [0]
    info = {'rounds': 0, 'pairs': 0, 'too_many_rows': 0, 'tested': []}
    while fresh:
        for i in fresh:
            boxes[i] = _box(rows[i], n_t)
        cand = set()
        for i in fresh:
            if boxes[i] is None:
                continue
            for j in sorted(alive):
                if j != i and group[j] == group[i] and boxes[j] is not None and _touch(boxes[i], boxes[j], tol):
                    cand.add((i, j) if key[i] < key[j] else (j, i))
        if not cand:
            break
        info['rounds'] += 1
        info['pairs'] += len(cand)
        taken, fresh = set(), []
        for p, q in sorted(cand, key=lambda pq: (key[pq[0]], key[pq[1]])):
            ok, va, vb = _pair_test(rows[p], rows[q], n_t, tol, knife)   # every candidate is tested, as on the device
            info['tested'].append((rows[p], rows[q], va, vb, ok))
            if not ok or p in taken or q in taken:
                continue
            u = _dedupe(numpy.vstack([rows[p][va], rows[q][vb]]), tol)
            if len(u) > MAX_ROWS:
                info['too_many_rows'] += 1
                continue
            taken.update((p, q))
            members.append(sorted(members[p] + members[q]))
            rows.append(u)
            boxes.append(None)
            key.append(min(key[p], key[q]))
            group.append(group[p])
            alive.add(len(members) - 1)
            fresh.append(len(members) - 1)
        alive -= taken
    final = sorted(alive, key=lambda i: key[i])
    info['knife'] = knife[0]
    info['groups'] = len(reps)
    sol = build_merged_solution(solution, [members[i] for i in final], [rows[i] if len(members[i]) > 1 else None for i in final], outputs)
    return sol, info


def pair_rejected(rows_p, rows_q, tol=1e-8):
    """The reference's pair test on two regions given as (E, f): True when their union is not convex (or not within tol)."""
    n_t = numpy.asarray(rows_p[0]).shape[1]
    up, _ = _unit(*rows_p, n_t)
    uq, _ = _unit(*rows_q, n_t)
    return not _pair_test(up, uq, n_t, tol, [0])[0]
