"""Plots of explicit solutions (reference: plot.py).  The polygons come from Solution.slice_2d, one device launch for all regions
(csrc/locate.hpp: k_slice_polygons), so a solution of any number of parameters can be drawn in a 2-D slice; the drawing itself
(plot_slice) takes an existing SolutionSlice and needs no device.  matplotlib and plotly are imported inside the functions, so that
importing ppopt_amd never needs them."""
import time
from math import atan2
from typing import List, Optional

import numpy

from .geometry.slice import SolutionSlice


def vertex_enumeration_2d(A: numpy.ndarray, b: numpy.ndarray, solver=None, tol: float = 1e-9) -> List[numpy.ndarray]:
    """The vertices of the 2-D polytope {x : A x <= b}, each once: every pair of rows solved as equalities (numpy, on the host) and
    kept where all rows hold within tol (1 + |b|).  The reference solves one LP per pair of rows and returns a vertex once per pair
    through it, so a vertex where three rows meet appears there three times; here it appears once.  ``solver`` is accepted for the
    reference's signature and not used."""
    A = numpy.asarray(A, dtype=float)
    b = numpy.asarray(b, dtype=float).reshape(-1)
    i, j = numpy.triu_indices(A.shape[0], k=1)
    M = numpy.stack([A[i], A[j]], axis=1)                                     # [pairs, 2, 2]
    det = M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]
    scale = numpy.linalg.norm(A[i], axis=1) * numpy.linalg.norm(A[j], axis=1)
    ok = numpy.abs(det) > tol * numpy.maximum(scale, 1e-300)
    if not numpy.any(ok):
        return []
    x = numpy.linalg.solve(M[ok], numpy.stack([b[i[ok]], b[j[ok]]], axis=1)[..., None])[..., 0]
    feas = numpy.all(x @ A.T - b <= tol * (1.0 + numpy.abs(b)), axis=1)
    out: List[numpy.ndarray] = []
    for v in x[feas]:
        if not any(numpy.max(numpy.abs(v - w)) <= tol * (1.0 + numpy.max(numpy.abs(w))) for w in out):
            out.append(v)
    return out


def sort_clockwise(vertices: List[numpy.ndarray]) -> List[numpy.ndarray]:
    """The vertices sorted by ascending atan2 about their mean -- counter-clockwise, despite the name the reference gives it."""
    center = sum(vertices, numpy.array([0.0, 0.0])) / len(vertices)
    return sorted(vertices, key=lambda x: atan2((x[1] - center[1]), (x[0] - center[0])))


def gen_vertices(solution, dims=(0, 1), fixed=None, box=None, device: int = 0) -> List[List[numpy.ndarray]]:
    """One vertex list per region of the solution, in the reference's order (ascending atan2 about the vertex mean), from one
    slice_2d; an empty list for a region that does not meet the slice.  For a solution of more than two parameters give ``fixed``."""
    sl = solution.slice_2d(dims=dims, fixed=fixed, box=box, device=device)
    return [[v for v in verts] for verts in sl.vertices]


def plot_slice(sl: SolutionSlice, ax=None, seed: Optional[int] = None, cmap: str = 'Paired', alpha: float = .8):
    """Draws the full-dimensional polygons of a SolutionSlice as one PatchCollection on ``ax`` (a new figure when None), coloured at
    random like the reference's parametric_plot, and limits the axes to the slice's box.  Returns the axes."""
    import matplotlib
    from matplotlib import pyplot
    from matplotlib.collections import PatchCollection
    from matplotlib.patches import Polygon

    if seed is None:
        seed = time.time_ns()
    if ax is None:
        _, ax = pyplot.subplots()
    full = numpy.flatnonzero(sl.full())
    patches = [Polygon(sl.vertices[k], closed=True) for k in full]
    rng = numpy.random.default_rng(seed)
    p = PatchCollection(patches, cmap=matplotlib.colormaps[cmap], alpha=alpha, edgecolors='black', linewidths=1)
    p.set_array(100 * rng.random(len(patches)))
    ax.add_collection(p)
    ax.set_xlim(sl.box[0], sl.box[2])
    ax.set_ylim(sl.box[1], sl.box[3])
    if sl.dims is not None:
        ax.set_xlabel(f'theta_{sl.dims[0]}')
        ax.set_ylabel(f'theta_{sl.dims[1]}')
    return ax


def parametric_plot(solution, save_path: Optional[str] = None, show=True, save_format: str = 'png', seed: Optional[int] = None,
                    fixed=None, dims=(0, 1), box=None) -> None:
    """Draws the regions of the solution with matplotlib: a 2-D solution as it is, a solution of more parameters in the slice that
    holds ``dims`` free and the other parameters at ``fixed``.  Without ``fixed`` a solution that is not 2-D is refused with a message,
    as in the reference.  ``save_path``: the figure is written to save_path + '.' + save_format."""
    from matplotlib import pyplot

    if solution.theta_dim() != 2 and fixed is None:
        print(f"Solution is not 2D, the dimensionality of the solution is {solution.theta_dim()}")
        return
    sl = solution.slice_2d(dims=dims, fixed=fixed, box=box)
    ax = plot_slice(sl, seed=seed)
    if save_path is not None:
        pyplot.savefig(save_path + "." + save_format, dpi=1000, format=save_format)
    if show:
        pyplot.show()
    pyplot.close(ax.figure)


def parametric_plot_1D(solution, save_path: Optional[str] = None, show=True, save_format: str = 'png',
                       legend: Optional[List[str]] = None, plot_subset: Optional[List[int]] = None, theta_0=None, direction=None,
                       t_range=None) -> None:
    """Plots x*(theta) of every region along a line with matplotlib, one colour per variable: a 1-D solution over its parameter range,
    a solution of more parameters along theta_0 + direction t.  Without ``direction`` a solution that is not 1-D is refused with a
    message, as in the reference.  ``plot_subset``: the variables to draw; ``legend``: their labels."""
    import matplotlib
    from matplotlib import pyplot

    n_t = solution.theta_dim()
    if n_t != 1 and direction is None:
        print(f"Solution is not 1D, the dimensionality of the solution is {n_t}")
        return
    theta_0 = numpy.zeros(n_t) if theta_0 is None else theta_0
    direction = numpy.ones(1) if direction is None else direction
    ls = solution.slice_1d(theta_0, direction, t_range=t_range)
    n_x = ls.x_start.shape[1]
    if plot_subset is None:
        plot_subset = list(range(n_x))
    _, ax = pyplot.subplots()
    cm = matplotlib.colormaps['rainbow']
    colors = [cm(x_i) for x_i in numpy.linspace(0, 1, n_x)]
    for k in numpy.flatnonzero(ls.full()):
        for v in plot_subset:
            ax.plot(ls.intervals[k], [ls.x_start[k, v], ls.x_end[k, v]], solid_capstyle='round', color=colors[v])
    if legend is not None:
        ax.legend(legend)
    if save_path is not None:
        pyplot.savefig(save_path + "." + save_format, dpi=1000, format=save_format)
    if show:
        pyplot.show()
    pyplot.close(ax.figure)


def plotly_plot(solution, save_path: Optional[str] = None, show=True, save_format: str = 'png', fixed=None, dims=(0, 1),
                box=None) -> None:
    """The regions of the solution (or of its slice, as parametric_plot) as an interactive plotly figure; ``save_path``: an image in
    ``save_format`` and an html copy.  Raises ImportError when plotly is not installed."""
    try:
        import plotly.graph_objects as go
    except ImportError as e:
        raise ImportError('plotly_plot needs the plotly package, which is not installed') from e
    fig = go.Figure()
    for i, region_v in enumerate(gen_vertices(solution, dims=dims, fixed=fixed, box=box)):
        fig.add_trace(go.Scatter(x=[v[0] for v in region_v], y=[v[1] for v in region_v], fill="toself", name=f'Critical Region {i}'))
    fig.update_layout(autosize=False, width=1000, height=1000)
    fig.update_layout(hoverlabel={'bgcolor': 'white'})
    if save_path is not None:
        fig.write_image(save_path + "." + save_format)
        fig.write_html(save_path + ".html", include_plotlyjs=False, full_html=False)
    if show:
        fig.show()
