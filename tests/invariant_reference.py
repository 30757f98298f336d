"""An independent CPU statement of the backward exit cells of DESIGN §3.23 (numpy and scipy's HiGHS, on transition_reference.pulled_back
and chebyshev, as exit_reference.py): the same definitions, thresholds and order as ppopt_amd/invariant_set.py, none of its code.

  backward_reference(polys, Phi, phi, predecessors, cells0, tol, max_steps) -> (cells, items, converged)
      cells0: [(source, rows)] the cells of step 0.  cells: dicts with source, step, parent (index into cells, -1 at step 0), rows
      [m, n_t + 1] unit [o | n], wide (its radius run, or an ancestor's, was unbounded), lineage (the step-0 cell, then the region of
      every later step: a cell's name, whatever the order) and knife (the item that made it, or one of its ancestors, was a KNIFE ITEM), step by step, a step in item order.  items: dicts
      with step, parent, region, outcome ('none', 'cell', 'empty'), knife.  The items of a step are ordered by parent cell, then by region
      ascending.
  A KNIFE ITEM: its radius decision or the redundancy run of one of its rows ended within KNIFE of tol, or a pulled-back row norm lay
  within a factor 10 of its threshold.  The device, whose simplex rounds otherwise, may legitimately decide there the other way.
  reduce_in_order(rows, tol) -> (kept mask, wide, knife): one LP per row, in row order: row k goes when the rows still live, with row k
      reversed, have a radius <= tol; an unbounded run keeps the row.
  replay_exit_step(polys, Phi, phi, thetas, cap) -> [n] the first step (1-based) at which some trajectory of the point lands in no
      polytope, over every choice of a polytope that holds the state (the polytopes of a synthetic set overlap), 0 when none does within
      cap steps, -1 outside every polytope; and the smallest |margin| of any membership decision on the way.
"""
import numpy

import transition_reference as tref

KNIFE = tref.KNIFE


def reduce_in_order(rows, tol):
    live = numpy.ones(len(rows), dtype=bool)
    wide = knife = False
    for k in range(len(rows)):
        live[k] = False
        open_, r, _ = tref.chebyshev(numpy.vstack([rows[live], -rows[k][None]]))
        if open_:
            wide = True
            live[k] = True
            continue
        knife = knife or abs(r - tol) <= KNIFE
        live[k] = r > tol
    return live, wide, knife


def backward_reference(polys, Phi, phi, predecessors, cells0, tol=1e-8, max_steps=64):
    cells = [dict(source=int(s), step=0, parent=-1, rows=numpy.asarray(r, dtype=float), wide=False, lineage=(c,), knife=False)
             for c, (s, r) in enumerate(cells0)]
    items = []
    lo, hi, step, converged = 0, len(cells), 0, False
    while True:
        todo = [(c, int(i)) for c in range(lo, hi) for i in sorted(set(int(p) for p in predecessors[cells[c]['source']]))]
        if not todo:
            converged = True
            break
        if step == max_steps:
            break
        fresh = []
        for c, i in todo:
            Q = cells[c]
            back, empty, knife = tref.pulled_back(Q['rows'], numpy.asarray(Phi[i], dtype=float), numpy.asarray(phi[i], dtype=float), tol)
            item = dict(step=step + 1, parent=c, region=i, outcome='empty', knife=bool(knife))
            items.append(item)
            if empty:
                continue
            rows = numpy.vstack([numpy.asarray(polys[i], dtype=float), back])
            open_, r, _ = tref.chebyshev(rows)
            if not open_ and abs(r - tol) <= KNIFE:
                item['knife'] = True
            if not open_ and not r > tol:
                item['outcome'] = 'none'
                continue
            kept, _, kn = reduce_in_order(rows, tol)
            item['knife'] = item['knife'] or kn
            item['outcome'] = 'cell'
            fresh.append(dict(source=i, step=step + 1, parent=c, rows=rows[kept], wide=bool(open_ or Q['wide']),
                              lineage=Q['lineage'] + (i,), knife=bool(item['knife'] or Q['knife'])))
        if not fresh:
            converged = True
            break
        cells.extend(fresh)
        lo, hi, step = hi, hi + len(fresh), step + 1
    return cells, items, converged


def replay_exit_step(polys, Phi, phi, thetas, cap):
    th = numpy.asarray(thetas, dtype=float)
    n = len(th)
    Phi, phi = numpy.asarray(Phi, dtype=float), numpy.asarray(phi, dtype=float)
    off = numpy.concatenate([[0], numpy.cumsum([len(p) for p in polys])])
    rows = numpy.vstack(polys)

    def margins(x):      # [polytopes, states]: the largest row violation, <= 0 inside
        return numpy.maximum.reduceat(rows[:, 1:] @ x.T - rows[:, :1], off[:-1], axis=0)

    out = numpy.zeros(n, dtype=numpy.int64)
    near = numpy.full(n, numpy.inf)
    m = margins(th)
    numpy.minimum.at(near, numpy.arange(n), numpy.min(numpy.abs(m), axis=0))
    out[~(m <= 0.0).any(axis=0)] = -1
    owner, state = numpy.flatnonzero(out == 0), th[out == 0]
    for t in range(1, cap + 1):
        if not len(owner):
            break
        inside = margins(state) <= 0.0                       # every branch: a polytope that holds the state
        reg, k = numpy.nonzero(inside)
        img = numpy.einsum('ktl,kl->kt', Phi[reg], state[k]) + phi[reg]
        own = owner[k]
        mi = margins(img)
        numpy.minimum.at(near, own, numpy.min(numpy.abs(mi), axis=0))
        gone = ~(mi <= 0.0).any(axis=0)
        out[numpy.unique(own[gone])] = t
        keep = out[own] == 0
        owner, state = own[keep], img[keep]
        if len(owner):                                       # the same state reached twice is one branch
            _, first = numpy.unique(numpy.column_stack([owner, state]), axis=0, return_index=True)
            owner, state = owner[first], state[first]
    return out, near
