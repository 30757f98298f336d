"""An independent CPU statement of the law gap of DESIGN §3.26 (numpy and scipy's HiGHS): the same definition as ppopt_amd/compare.py,
none of its code.  A pair whose radius lies within KNIFE of tol is recorded as knife: it may legitimately differ from the device, whose
simplex rounds otherwise.

  pair_reference(rows_i, rows_j, law_i, law_j, tol)   rows: [m, n + 1] unit rows [o | n]; laws: [K, n + 1] = [b | A]
  gap_reference(polys, laws, pairs, tol)              {(i, j): pair_reference(...)} over one table of polytopes
"""
import numpy
from scipy.optimize import linprog

KNIFE = 1e-9          # the value of overlap_reference.py
_OPT = {'primal_feasibility_tolerance': 1e-10, 'dual_feasibility_tolerance': 1e-10}


def _lp(c, A, b):
    """(status, optimum) of min c.x over A x <= b, x free; status 0 optimal, 3 unbounded"""
    r = linprog(c, A_ub=A, b_ub=b, bounds=[(None, None)] * len(c), method='highs-ds', options=_OPT)
    if r.status not in (0, 3):
        raise RuntimeError(f'LP ended with status {r.status}')
    return r.status, (float(r.fun) if r.status == 0 else None)


def radius(rows):
    """the largest t with n.theta + t <= o for all rows; +inf when the LP is unbounded"""
    n = rows.shape[1] - 1
    st, fun = _lp(numpy.append(numpy.zeros(n), -1.0), numpy.hstack([rows[:, 1:], numpy.ones((len(rows), 1))]), rows[:, 0])
    return numpy.inf if st == 3 else -fun


def pair_reference(rows_i, rows_j, law_i, law_j, tol=1e-8):
    """dict: radius, meets, knife, gap, row, lo [K], hi [K], flag, lps (the radius LP and the range LPs that ran), constant (rows)"""
    both = numpy.vstack([rows_i, rows_j])
    K = len(law_i)
    r = radius(both)
    out = {'radius': r, 'knife': bool(numpy.isfinite(r) and abs(r - tol) <= KNIFE), 'meets': bool(r > tol), 'gap': numpy.nan, 'row': -1,
           'lo': numpy.full(K, numpy.nan), 'hi': numpy.full(K, numpy.nan), 'flag': 0, 'lps': 1, 'constant': 0}
    if numpy.isinf(r):
        out.update(gap=numpy.inf, flag=1)
        return out
    if not out['meets']:
        return out
    for k in range(K):
        d = law_i[k, 1:] - law_j[k, 1:]
        c0 = law_i[k, 0] - law_j[k, 0]
        if not numpy.any(d != 0.0):
            out['lo'][k] = out['hi'][k] = c0
            out['constant'] += 1
            continue
        st, fun = _lp(d, both[:, 1:], both[:, 0])
        out['lo'][k] = -numpy.inf if st == 3 else fun + c0
        st, fun = _lp(-d, both[:, 1:], both[:, 0])
        out['hi'][k] = numpy.inf if st == 3 else -fun + c0
        out['lps'] += 2
    per_row = numpy.maximum(-out['lo'], out['hi'])
    out['gap'] = float(per_row.max())
    out['row'] = int(numpy.argmax(per_row))         # the lowest row that attains it
    out['flag'] = int(numpy.isinf(out['gap']))
    return out


def gap_reference(polys, laws, pairs, tol=1e-8):
    return {(int(i), int(j)): pair_reference(polys[i], polys[j], laws[i], laws[j], tol) for i, j in pairs}
