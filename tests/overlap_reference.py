"""An independent CPU statement of the overlap removal of DESIGN §3.19 (numpy and scipy's HiGHS): the same rules, order and thresholds
as ppopt_amd/overlap.py, none of its code.  Every LP value within KNIFE of the threshold it is compared with is recorded: a case
with such a record may legitimately differ from the device, whose simplex rounds otherwise.

  partition_reference(polys, g, h, tol, value_tol)  polys: list of [m, n + 1] unit rows [o | n]; affine values g_i.theta + h_i
  reduce_reference(solution, tol, value_tol)        the same from a Solution (regions E, f and the objective along each region's law)
"""
import numpy
from scipy.optimize import linprog

KNIFE = 1e-9
MAX_ROWS = 256
_OPT = {'primal_feasibility_tolerance': 1e-10, 'dual_feasibility_tolerance': 1e-10}


class Record:
    def __init__(self):
        self.knife = []      # (what, value, threshold)
        self.lps = 0

    def near(self, what, value, thr):
        if numpy.isfinite(value) and abs(value - thr) <= KNIFE:
            self.knife.append((what, float(value), float(thr)))


def _lp(rec, c, A, b):
    """(status, optimum, x) of min c.x over A x <= b, x free; status 0 optimal, 3 unbounded, 2 infeasible"""
    rec.lps += 1
    r = linprog(c, A_ub=A, b_ub=b, bounds=[(None, None)] * len(c), method='highs-ds', options=_OPT)
    return r.status, (r.fun if r.status == 0 else None), (r.x if r.status == 0 else None)


def radius(rec, rows):
    """(open, r): the largest t with n.theta + t <= o for all rows; open when the LP is unbounded"""
    n = rows.shape[1] - 1
    st, fun, _ = _lp(rec, numpy.append(numpy.zeros(n), -1.0), numpy.hstack([rows[:, 1:], numpy.ones((len(rows), 1))]), rows[:, 0])
    if st == 0:
        return False, -fun
    if st == 3:
        return True, numpy.inf
    raise RuntimeError(f'radius LP ended with status {st}')


def depth_range(rec, rows, cut):
    """(open, d_min, d_max) of d(theta) = o - n.theta over the rows"""
    lo_st, lo, _ = _lp(rec, cut[1:], rows[:, 1:], rows[:, 0])        # min n.theta
    hi_st, hi, _ = _lp(rec, -cut[1:], rows[:, 1:], rows[:, 0])       # -max n.theta
    if lo_st != 0 or hi_st != 0:
        return True, -numpy.inf, numpy.inf
    return False, cut[0] + hi, cut[0] - lo


def box_of(rec, rows):
    n = rows.shape[1] - 1
    lo, hi = numpy.empty(n), numpy.empty(n)
    for t in range(n):
        e = numpy.zeros(n)
        e[t] = 1.0
        st, fun, _ = _lp(rec, e, rows[:, 1:], rows[:, 0])
        if st == 2:
            return None
        lo[t] = fun if st == 0 else -numpy.inf
        st, fun, _ = _lp(rec, -e, rows[:, 1:], rows[:, 0])
        hi[t] = -fun if st == 0 else numpy.inf
    return lo, hi


def partition_reference(polys, g, h, tol=1e-8, value_tol=1e-9, max_pieces=1 << 20):
    rec = Record()
    polys = [numpy.asarray(p, dtype=float) for p in polys]
    R = len(polys)
    n = polys[0].shape[1] - 1
    g = numpy.asarray(g, dtype=float).reshape(R, n)
    h = numpy.asarray(h, dtype=float).reshape(R)
    boxes = [box_of(rec, p) for p in polys]
    g_thr = value_tol * (1.0 + max(numpy.linalg.norm(g[i]) for i in range(R)))
    h_thr = value_tol * (1.0 + max(abs(h[i]) for i in range(R)))
    verdicts, values = {}, {}
    cutters = [[] for _ in range(R)]
    for i in range(R):
        for j in range(i + 1, R):
            if boxes[i] is None or boxes[j] is None:
                continue
            with numpy.errstate(invalid='ignore'):
                ov = numpy.minimum(boxes[i][1], boxes[j][1]) - numpy.maximum(boxes[i][0], boxes[j][0])
            for v in ov:
                rec.near('box', v, tol)
            if not numpy.all(ov > tol):
                continue
            dg, dh = g[i] - g[j], h[i] - h[j]
            gn = numpy.linalg.norm(dg)
            flat = gn <= g_thr
            equal = flat and abs(dh) <= h_thr
            cut = None if flat else numpy.append(dh / gn, -dg / gn)
            both = numpy.vstack([polys[i], polys[j]])
            is_open, r = radius(rec, both)
            d_min = d_max = numpy.nan
            if is_open:
                verdict = 'EQUAL' if equal else ('CROSSING' if cut is not None else ('J_WINS' if dh > 0 else 'I_WINS'))
            else:
                rec.near('radius', r, tol)
                if r <= tol:
                    verdict = 'DISJOINT'
                elif equal:
                    verdict = 'EQUAL'
                else:
                    if cut is None:
                        d_open, d_min, d_max = False, numpy.copysign(numpy.inf, dh), numpy.copysign(numpy.inf, dh)
                    else:
                        d_open, d_min, d_max = depth_range(rec, both, cut)
                    if d_open:
                        verdict = 'CROSSING'
                    else:
                        rec.near('d_max', d_max, tol)
                        rec.near('d_min', d_min, -tol)
                        verdict = 'I_WINS' if d_max <= tol else ('J_WINS' if d_min >= -tol else 'CROSSING')
            verdicts[(i, j)] = verdict
            values[(i, j)] = (r, d_min, d_max)
            if verdict in ('EQUAL', 'J_WINS'):
                cutters[i].append((j, polys[j]))
            elif verdict == 'I_WINS':
                cutters[j].append((i, polys[i]))
            elif verdict == 'CROSSING':
                cutters[i].append((j, numpy.vstack([polys[j], cut])))
                cutters[j].append((i, numpy.vstack([polys[i], -cut])))
    pieces = [[] if boxes[i] is None else [(polys[i], True)] for i in range(R)]     # (rows, untouched)
    for c in cutters:
        c.sort(key=lambda jc: jc[0])
    for rnd in range(max((len(c) for c in cutters), default=0)):
        for i in range(R):
            if len(cutters[i]) <= rnd:
                continue
            C = cutters[i][rnd][1]
            nxt = []
            for P, whole in pieces[i]:
                is_open, r = radius(rec, numpy.vstack([P, C]))
                if not is_open:
                    rec.near('meets', r, tol)
                if not is_open and r <= tol:
                    nxt.append((P, whole))
                    continue
                cutting = []
                for k in range(len(C)):
                    cand = numpy.vstack([P] + cutting + [-C[k:k + 1]])
                    c_open, rk = radius(rec, cand)
                    if not c_open:
                        rec.near('cuts', rk, tol)
                    if c_open or rk > tol:
                        nxt.append((cand, False))
                        cutting.append(C[k:k + 1])
            pieces[i] = nxt
        if any(len(P) > MAX_ROWS for ps in pieces for P, _ in ps):
            raise ValueError(f'a piece has more than {MAX_ROWS} rows after round {rnd + 1}')
        if sum(len(ps) for ps in pieces) > max_pieces:
            raise ValueError(f'more than max_pieces = {max_pieces} pieces after round {rnd + 1}')
    return {'pieces': [P for ps in pieces for P, _ in ps], 'whole': [w for ps in pieces for _, w in ps],
            'sources': numpy.asarray([i for i in range(R) for _ in pieces[i]], dtype=numpy.int64),
            'vanished': [i for i in range(R) if not pieces[i]], 'verdicts': verdicts, 'values': values, 'knife': rec.knife, 'lps': rec.lps}


def unit(E, f):
    E = numpy.asarray(E, dtype=float)
    f = numpy.asarray(f, dtype=float).reshape(-1)
    nrm = numpy.sqrt((E * E).sum(axis=1))
    return numpy.column_stack([f / nrm, E / nrm[:, None]])


def affine_values(solution):
    """(g [R, n], h [R]) with J_i(theta) = g_i.theta + h_i + (a part common to all regions): the objective along each region's law at
    the origin and at the unit points"""
    P = solution.program
    n = P.num_t()
    g, h = [], []
    for r in solution.critical_regions:
        J = lambda th: float(P.evaluate_objective(r.evaluate(th.reshape(-1, 1)), th.reshape(-1, 1)))
        h.append(J(numpy.zeros(n)))
        g.append([J(numpy.eye(n)[k]) - h[-1] for k in range(n)])
    return numpy.asarray(g), numpy.asarray(h)


def reduce_reference(solution, tol=1e-8, value_tol=1e-9):
    g, h = affine_values(solution)
    return partition_reference([unit(r.E, r.f) for r in solution.critical_regions], g, h, tol, value_tol)
