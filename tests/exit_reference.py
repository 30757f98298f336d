"""An independent CPU statement of the exit sets of DESIGN §3.21 (numpy and scipy's HiGHS, on transition_reference.pulled_back and
chebyshev): the same definitions, thresholds and order as ppopt_amd/exit_sets.py, none of its code.

  exit_reference(polys, Phi, phi, successors, tol, regions)  -> (pieces, knife) of all regions or of ``regions`` only: pieces is a list
                                                     of (source, rows [m, n_t + 1] unit [o | n], wide, whole) in the order of ExitSets; knife the set of KNIFE REGIONS: regions where some
                                                     decision had |r - tol| <= KNIFE, or a pulled-back row norm lay within a factor 10 of
                                                     its threshold.  The device, whose simplex rounds otherwise, may legitimately decide
                                                     there the other way, and the pieces of such a region are not compared.
  successors_reference(polys, Phi, phi, tol)        every region's successors from transition_reference.graph_reference over all pairs
  exits(polys, Phi, phi, thetas, region)            per point: the signed margin by which its image leaves every polytope (the smallest,
                                                     over the polytopes, of the largest row violation): > 0 iff the image lies in none
"""
import numpy

import transition_reference as tref

KNIFE = tref.KNIFE


def _radius(rows, tol, state):
    """(above, wide) of the radius decision r > tol over the rows; an unbounded run counts as above and wide"""
    open_, r, _ = tref.chebyshev(rows)
    if open_:
        return True, True
    if abs(r - tol) <= KNIFE:
        state['knife'] = True
    return r > tol, False


def difference(piece, cutter, tol, state):
    """None when radius(piece n cutter) <= tol (the piece stays), else (children, wide): piece n {earlier cutting rows} n {reversed row
    k} for every row k of the cutter, in order, whose candidate has a radius above tol"""
    meets, wide = _radius(numpy.vstack([piece, cutter]), tol, state)
    if not meets:
        return None
    children, cutting = [], []
    for row in cutter:
        cand = numpy.vstack([piece] + cutting + [-row[None]])
        above, w = _radius(cand, tol, state)
        wide = wide or w
        if above:
            children.append(cand)
            cutting.append(row[None])
    return children, wide


def exit_reference(polys, Phi, phi, successors, tol=1e-8, regions=None):
    pieces, knife = [], set()
    for i in (range(len(polys)) if regions is None else sorted(int(r) for r in regions)):
        poly = polys[i]
        state = {'knife': False}
        live = [(numpy.asarray(poly, dtype=float), False, True)]
        for j in sorted(set(int(s) for s in successors[i])):
            back, empty, kn = tref.pulled_back(polys[j], numpy.asarray(Phi[i], dtype=float), numpy.asarray(phi[i], dtype=float), tol)
            state['knife'] = state['knife'] or kn
            if empty:
                continue
            nxt = []
            for rows, wide, whole in live:
                res = difference(rows, back, tol, state)
                if res is None:
                    nxt.append((rows, wide, whole))
                else:
                    nxt.extend((child, wide or res[1], False) for child in res[0])
            live = nxt
        if state['knife']:
            knife.add(i)
        pieces.extend((i, rows, wide, whole) for rows, wide, whole in live)
    return pieces, knife


def successors_reference(polys, Phi, phi, tol=1e-8):
    """(successors per region, the regions with a knife pair) over all R^2 pairs"""
    R = len(polys)
    got = tref.graph_reference(polys, Phi, phi, tol)
    succ = [[j for j in range(R) if got[(i, j)][0] != tref.NO_EDGE] for i in range(R)]
    return succ, {i for (i, _), v in got.items() if v[2]}


def exits(polys, Phi, phi, thetas, region):
    """[n]: min over the polytopes of max over its rows of n.(Phi_i theta + phi_i) - o, i = region[k]: positive iff the image of point k
    violates some row of every polytope"""
    img = numpy.einsum('ktl,kl->kt', numpy.asarray(Phi)[region], thetas) + numpy.asarray(phi)[region]
    out = numpy.full(len(thetas), numpy.inf)
    for rows in polys:
        out = numpy.minimum(out, numpy.max(img @ rows[:, 1:].T - rows[:, 0], axis=1))
    return out
