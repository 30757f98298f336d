"""An independent CPU statement of the forward cells of DESIGN §3.25 (numpy and scipy's HiGHS, on transition_reference.pulled_back and
chebyshev; the row rule is invariant_reference.reduce_in_order with the knife band of this file): the same definitions, thresholds and
order as ppopt_amd/reach.py, none of its code.

  next_map(Phi_i, phi_i, G, g) -> (P, s)
      P = Phi_i G, s = Phi_i g + phi_i by the explicit loop of the definition: every entry one sum over t ascending from 0.0 of plain
      IEEE products (Python floats: no contraction), so (G, g) can be compared bit for bit.
  forward_reference(polys, Phi, phi, successors, cells0, tol, max_steps) -> (cells, items, status)
      cells0: [(region, rows)] the cells of step 0.  cells: dicts with region, step, parent (index into cells, -1 at step 0), rows
      [m, n_t + 1] unit [o | n] over theta_0, G, g, wide (its radius run, or an ancestor's, was unbounded), lineage (the step-0 cell,
      then the region of every later step: a cell's name, whatever the order) and knife (the item that made it, or one of its
      ancestors, was a KNIFE ITEM), step by step, a step in item order.  items: dicts with step, parent, region, outcome ('none',
      'cell', 'empty'), knife, lps, wide (the unbounded runs of the item, every run taken to its end: a device run stops once t > tol and
      sees fewer).  The items of a step are ordered by parent cell, then by region ascending.  status: 'DONE' or 'EMPTY'.
  pack / unpack, set_reference, golden_path: the runs on exit_cases.SETS as recorded under tests/golden (python tests/forward_reference.py
      writes them; tests/test_forward_cpu.py checks the records against a fresh run).
  A KNIFE ITEM: its radius decision or the redundancy run of one of its rows ended within KNIFE of tol, or a pulled-back row norm lay
  within a factor 10 of its threshold.  The device, whose simplex rounds otherwise, may legitimately decide there the other way.
  replay(polys, Phi, phi, thetas, steps) -> (theta [steps + 1, n, n_t], region [steps + 1, n] (-1 from the step at which the state lies
      in no polytope), near [n] the smallest |margin| of any membership decision along the trajectory, while it lasted): for polytopes
      that do not overlap (the first polytope that holds the state acts).
"""
import numpy

import transition_reference as tref

KNIFE = 5e-7


def next_map(Phi_i, phi_i, G, g):
    n = len(phi_i)
    P, s = numpy.zeros((n, n)), numpy.zeros(n)
    for r in range(n):
        for k in range(n):
            acc = 0.0
            for t in range(n):
                acc = acc + float(Phi_i[r][t]) * float(G[t][k])
            P[r, k] = acc
        acc = 0.0
        for t in range(n):
            acc = acc + float(Phi_i[r][t]) * float(g[t])
        s[r] = acc + float(phi_i[r])
    return P, s


def reduce_in_order(rows, tol):
    """invariant_reference.reduce_in_order with the band of this file: (kept, unbounded runs, knife)"""
    live = numpy.ones(len(rows), dtype=bool)
    wide, knife = 0, False
    for k in range(len(rows)):
        live[k] = False
        open_, r, _ = tref.chebyshev(numpy.vstack([rows[live], -rows[k][None]]))
        if open_:
            wide += 1
            live[k] = True
            continue
        knife = knife or abs(r - tol) <= KNIFE
        live[k] = r > tol
    return live, wide, knife


def forward_reference(polys, Phi, phi, successors, cells0, tol=1e-8, max_steps=8):
    n = numpy.asarray(polys[0]).shape[1] - 1
    cells = [dict(region=int(i), step=0, parent=-1, rows=numpy.asarray(r, dtype=float), G=numpy.eye(n), g=numpy.zeros(n), wide=False, lineage=(c,),
                  knife=False) for c, (i, r) in enumerate(cells0)]
    items = []
    lo, hi, step, status = 0, len(cells), 0, 'DONE'
    if not cells:
        return cells, items, 'EMPTY'
    while step < max_steps:
        fresh = []
        for c in range(lo, hi):
            Q = cells[c]
            i = Q['region']
            succ = sorted(set(int(j) for j in successors[i]))
            if not succ:
                continue
            P, s = next_map(numpy.asarray(Phi[i], dtype=float), numpy.asarray(phi[i], dtype=float), Q['G'], Q['g'])
            for j in succ:
                back, empty, knife = tref.pulled_back(polys[j], P, s, tol)
                item = dict(step=step + 1, parent=c, region=j, outcome='empty', knife=bool(knife), lps=0, wide=0)
                items.append(item)
                if empty:
                    continue
                rows = numpy.vstack([Q['rows'], back])
                open_, r, _ = tref.chebyshev(rows)
                item['lps'], item['wide'] = 1, int(open_)
                if not open_ and abs(r - tol) <= KNIFE:
                    item['knife'] = True
                if not open_ and not r > tol:
                    item['outcome'] = 'none'
                    continue
                kept, wide, kn = reduce_in_order(rows, tol)
                item['lps'] += len(rows)
                item['wide'] += wide
                item['knife'] = item['knife'] or kn
                item['outcome'] = 'cell'
                fresh.append(dict(region=j, step=step + 1, parent=c, rows=rows[kept], G=P, g=s, wide=bool(open_ or Q['wide']),
                                  lineage=Q['lineage'] + (j,), knife=bool(item['knife'] or Q['knife'])))
        if not fresh:
            status = 'EMPTY'
            break
        cells.extend(fresh)
        lo, hi, step = hi, hi + len(fresh), step + 1
    return cells, items, status


_OUTCOMES = ('none', 'cell', 'empty')


def pack(cells, items, status):
    """a reference run as flat arrays (what tests/golden/forward_set_*.npz holds per case; the lineage follows from region and parent)"""
    off = numpy.concatenate([[0], numpy.cumsum([len(c['rows']) for c in cells])]).astype(numpy.int64)
    return {'cell_off': off, 'cell_rows': numpy.vstack([c['rows'] for c in cells]), 'region': numpy.asarray([c['region'] for c in cells], dtype=numpy.int32),
            'step': numpy.asarray([c['step'] for c in cells], dtype=numpy.int32), 'parent': numpy.asarray([c['parent'] for c in cells], dtype=numpy.int32),
            'G': numpy.asarray([c['G'] for c in cells]), 'g': numpy.asarray([c['g'] for c in cells]),
            'wide': numpy.asarray([c['wide'] for c in cells], dtype=bool), 'knife': numpy.asarray([c['knife'] for c in cells], dtype=bool),
            'item_parent': numpy.asarray([i['parent'] for i in items], dtype=numpy.int32),
            'item_region': numpy.asarray([i['region'] for i in items], dtype=numpy.int32),
            'item_outcome': numpy.asarray([_OUTCOMES.index(i['outcome']) for i in items], dtype=numpy.int8),
            'item_knife': numpy.asarray([i['knife'] for i in items], dtype=bool), 'item_lps': numpy.asarray([i['lps'] for i in items], dtype=numpy.int32),
            'item_wide': numpy.asarray([i['wide'] for i in items], dtype=numpy.int32), 'status': numpy.asarray(status)}


def unpack(z):
    """(cells, items, status) of pack's arrays"""
    cells = []
    for c in range(len(z['region'])):
        parent = int(z['parent'][c])
        cells.append(dict(region=int(z['region'][c]), step=int(z['step'][c]), parent=parent, rows=z['cell_rows'][z['cell_off'][c]:z['cell_off'][c + 1]],
                          G=z['G'][c], g=z['g'][c], wide=bool(z['wide'][c]), knife=bool(z['knife'][c]),
                          lineage=(c,) if parent < 0 else cells[parent]['lineage'] + (int(z['region'][c]),)))
    items = [dict(step=cells[int(p)]['step'] + 1, parent=int(p), region=int(j), outcome=_OUTCOMES[int(o)], knife=bool(k), lps=int(n), wide=int(w))
             for p, j, o, k, n, w in zip(z['item_parent'], z['item_region'], z['item_outcome'], z['item_knife'], z['item_lps'], z['item_wide'])]
    return cells, items, str(z['status'])


def replay(polys, Phi, phi, thetas, steps):
    th = numpy.asarray(thetas, dtype=float)
    n, n_t = th.shape
    Phi, phi = numpy.asarray(Phi, dtype=float), numpy.asarray(phi, dtype=float)
    off = numpy.concatenate([[0], numpy.cumsum([len(p) for p in polys])])
    rows = numpy.vstack(polys)
    theta = numpy.full((steps + 1, n, n_t), numpy.nan)
    region = numpy.full((steps + 1, n), -1, dtype=numpy.int64)
    near = numpy.full(n, numpy.inf)
    alive = numpy.ones(n, dtype=bool)
    x = th.copy()
    for k in range(steps + 1):
        idx = numpy.flatnonzero(alive)
        if not len(idx):
            break
        m = numpy.maximum.reduceat(rows[:, 1:] @ x[idx].T - rows[:, :1], off[:-1], axis=0)      # [polytopes, states], <= 0 inside
        near[idx] = numpy.minimum(near[idx], numpy.min(numpy.abs(m), axis=0))
        inside = m <= 0.0
        has = inside.any(axis=0)
        reg = inside.argmax(axis=0)
        theta[k, idx[has]] = x[idx[has]]
        region[k, idx[has]] = reg[has]
        alive[idx[~has]] = False
        go = idx[has]
        x[go] = numpy.einsum('ktl,kl->kt', Phi[reg[has]], x[go]) + phi[reg[has]]
    return theta, region, near


def golden_path(case):
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', f'forward_set_n{case[0]}_seed{case[1]}.npz')


def set_reference(case, tol, steps):
    """the arrays of pack plus succ_off, succ_idx (the reference graph) for exit_cases.synthetic_set(*case) from step 0 = the polytopes"""
    import exit_cases as xc
    import exit_reference as xref
    polys, Phi, phi = xc.synthetic_set(*case)
    succ, _ = xref.successors_reference(polys, Phi, phi, tol)
    out = pack(*forward_reference(polys, Phi, phi, succ, list(enumerate(polys)), tol, steps))
    out['succ_off'] = numpy.concatenate([[0], numpy.cumsum([len(s) for s in succ])]).astype(numpy.int64)
    out['succ_idx'] = numpy.asarray([j for s in succ for j in s], dtype=numpy.int32)
    return out


if __name__ == '__main__':      # python tests/forward_reference.py: writes the recorded reference runs of forward_cases.SETS
    import forward_cases as fc
    for case in fc.SETS:
        z = set_reference(case, fc.SET_TOL, fc.SET_STEPS)
        numpy.savez_compressed(golden_path(case), **z)
        print(case, len(z['item_parent']), 'items,', int(z['item_knife'].sum()), 'knife,', numpy.bincount(z['step']).tolist(), 'cells per step')
