"""The host side that invariant_set.backward_exit_cells and reach.forward_cells share: both hand polytopes with
maps, an adjacency and the cells of step 0 to one library call that runs every step.  Here: the argument checks, the adjacency as a
CSR, and the stats; the checks of the polytopes and their maps come from _pairs.py.  Host only; nothing here touches the library."""
import time

import numpy

from ._pairs import MAX_ROWS, check_polytopes, check_scalars, map_entries

MAX_TABLE_DOUBLES = 1 << 26     # the default capacity of the cell table, in doubles (max_rows_total = this // (n_t + 1))


def adjacency_csr(who, name, lists, R, void=()):
    """(adj_off [R + 1] int64, adj_idx int32) of ``lists`` (``name`` in the refusal), one index list per polytope: every list ascending,
    once each, without the ``void`` polytopes.  One sweep over all lists: a solution has thousands of regions."""
    lens = numpy.asarray([len(p) for p in lists], dtype=numpy.int64)
    flat = numpy.concatenate([numpy.asarray(p, dtype=numpy.int64).reshape(-1) for p in lists]) if lens.sum() else numpy.zeros(0, dtype=numpy.int64)
    if len(flat) and (flat.min() < 0 or flat.max() >= R):
        raise ValueError(f'{who}: {name} must name polytopes 0..{R - 1}')
    owner = numpy.repeat(numpy.arange(R), lens)
    order = numpy.lexsort((flat, owner))
    flat, owner = flat[order], owner[order]
    keep = numpy.ones(len(flat), dtype=bool)
    keep[1:] = (flat[1:] != flat[:-1]) | (owner[1:] != owner[:-1])
    if len(void):
        dead = numpy.zeros(R, dtype=bool)
        dead[numpy.asarray(list(void), dtype=numpy.int64)] = True
        keep &= ~dead[flat]
    return numpy.concatenate([[0], numpy.cumsum(numpy.bincount(owner[keep], minlength=R))]).astype(numpy.int64), flat[keep].astype(numpy.int32)


def check_cell_call(who, row_off, ef_rows, Phi, phi, n_t, adj_name, adjacency, cell_off, cell_rows, reg_name, per_cell, cell_reg, tol, max_steps,
                    max_cells, max_rows_total, void=()):
    """Every ValueError of the two calls but the forward one's cell_point, in their one order.  ``adj_name`` ('predecessors'), ``reg_name``
    ('cell_source') and ``per_cell`` ('one source') are the caller's words in the refusals.  The arrays the library call takes:
    (off, ef, Phi, phi, adj_off, adj_idx, cell_off, cell_rows, cell_reg, max_rows_total), max_rows_total with its default filled in."""
    check_scalars(who, n_t, tol)
    if int(max_steps) < 0:
        raise ValueError(f'{who}: max_steps must be >= 0')
    if int(max_cells) < 1:
        raise ValueError(f'{who}: max_cells must be >= 1')
    if max_rows_total is None:
        max_rows_total = MAX_TABLE_DOUBLES // (n_t + 1)
    if int(max_rows_total) < 1:
        raise ValueError(f'{who}: max_rows_total must be >= 1')
    Phi, phi = numpy.ascontiguousarray(Phi, dtype=numpy.float64), numpy.ascontiguousarray(phi, dtype=numpy.float64)
    off, ef, _, R = check_polytopes(who, row_off, ef_rows, n_t, extra=map_entries(Phi, phi, n_t), word='maps')
    if len(adjacency) != R:
        raise ValueError(f'{who}: {adj_name} needs one index list per polytope')
    adj_off, adj_idx = adjacency_csr(who, adj_name, adjacency, R, void)
    coff = numpy.ascontiguousarray(cell_off, dtype=numpy.int64).reshape(-1)
    crow = numpy.ascontiguousarray(cell_rows, dtype=numpy.float64).reshape(-1, n_t + 1)
    creg = numpy.ascontiguousarray(cell_reg, dtype=numpy.int64).reshape(-1)
    if len(coff) != len(creg) + 1 or coff[0] != 0 or coff[-1] != len(crow):
        raise ValueError(f'{who}: cell_off [cells + 1] must run from 0 to the number of rows of cell_rows, with {per_cell} per cell')
    if len(creg):
        c_counts = numpy.diff(coff)
        if c_counts.min() < 1 or c_counts.max() > MAX_ROWS:
            raise ValueError(f'{who}: every cell needs 1..{MAX_ROWS} rows')
        if creg.min() < 0 or creg.max() >= R:
            raise ValueError(f'{who}: {reg_name} must name polytopes 0..{R - 1}')
        if not numpy.all(numpy.isfinite(crow)):
            raise ValueError(f'{who}: cell rows must be finite')
        if len(creg) > int(max_cells) or len(crow) > int(max_rows_total):
            raise ValueError(f'{who}: the cells of step 0 exceed max_cells = {int(max_cells)} or max_rows_total = {int(max_rows_total)}')
    return off, ef, Phi, phi, adj_off, adj_idx, coff, crow, creg, int(max_rows_total)


def new_stats(n_cells0):
    return {'items': 0, 'cells': 0, 'empty': 0, 'lps': 0, 'pivots': 0, 'wide': 0, 'device_ms': 0.0, 'step_ms': [], 'cells_per_step': [n_cells0]}


def fill_stats(stats, r, max_steps, t_call, t_start):
    """the counters and times of the library call's result r (started at t_call) into stats; wall_ms since t_start"""
    for k in ('items', 'cells', 'empty', 'lps', 'pivots', 'wide'):
        stats[k] = r['stats'][k]
    stats['device_ms'] += r['stats']['ms']
    stats['call_ms'] = (time.perf_counter() - t_call) * 1e3
    stats['step_ms'] = [float(v) for v in r['step_ms'][:min(r['steps'] + 1, int(max_steps))]]
    stats['cells_per_step'] = [int(v) for v in r['cells_per_step']]
    stats['wall_ms'] = (time.perf_counter() - t_start) * 1e3
