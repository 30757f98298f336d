"""Polytope: the pair {x : A x <= b} (reference: geometry/polytope.py)."""
import numpy


class Polytope:
    """A convex polytope {x : A x <= b} in n dimensions."""

    def __init__(self, A: numpy.ndarray, b: numpy.ndarray):
        self.A = A
        self.b = b

    def rows(self):
        """([b | A] as one [m, n+1] float64 array) -- the stacking of mpc_hit_and_run and of the locator's [f | E] rows."""
        b = numpy.asarray(self.b, dtype=numpy.float64).reshape(-1, 1)
        A = numpy.asarray(self.A, dtype=numpy.float64)
        if A.ndim != 2 or A.shape[0] != b.shape[0]:
            raise ValueError(f'Polytope: A has shape {A.shape} but b has {b.shape[0]} rows')
        return numpy.hstack([b, A])

    def reduced(self, tol: float = 1e-8, device: int = 0) -> 'Polytope':
        """This polytope without its redundant rows (geometry.reduce): the rows are scaled to unit normals for the test
        (a zero row is a ValueError) and the kept ones are returned as they are here, in order.  A polytope of Chebyshev radius <= tol
        comes back unchanged."""
        from .reduce import reduced_polytope
        return reduced_polytope(self, tol=tol, device=device)

    def project(self, keep, tol: float = 1e-8, device: int = 0) -> 'Polytope':
        """The projection of this polytope onto the coordinates ``keep``, in their order, without redundant rows (geometry.project,
        DESIGN §3.24): the rows are scaled to unit normals first (a zero row is a ValueError) and the result has unit rows.  The whole
        space comes back as a Polytope without rows; a projection that is thin (Chebyshev radius <= tol, or empty) or needs more than
        512 rows at a step is a ValueError that names the status and the peak row count."""
        from .project import projected_polytope
        return projected_polytope(self, keep, tol=tol, device=device)

    def support(self, directions, tol: float = 1e-8, device: int = 0):
        """(values, args): h(d) = max {d.x : x in this polytope} for every row d of ``directions`` [k, n] and a point that attains it
        (geometry.support); one direction [n] gives one value and one point.  The rows are scaled to unit normals first (a
        zero row is a ValueError); the values are those of the directions as given.  +inf: the polytope is unbounded along d (or the
        run met the pivot cap); NaN: the polytope is thin (Chebyshev radius <= tol)."""
        from .support import polytope_support
        return polytope_support(self, directions, tol=tol, device=device)

    def erode(self, Q: 'Polytope', E=None, tol: float = 1e-8, reduce_rows: bool = True, device: int = 0) -> 'Polytope':
        """The Pontryagin difference {x : x + E q in this polytope for every q in Q} (geometry.support.pontryagin_difference, DESIGN
        §3.28): unit rows [o_k - h_Q(E' n_k) | n_k], without the redundant ones unless ``reduce_rows`` is off.  ``E``: [n, n_q], None
        for Q in this polytope's space.  ValueError that names the status for a difference that is EMPTY (Q unbounded where this
        polytope is bounded) or THIN (Chebyshev radius <= tol, or empty), and for a thin Q."""
        from .support import eroded_polytope
        return eroded_polytope(self, Q, E=E, tol=tol, reduce_rows=reduce_rows, device=device)

    def contains_polytope(self, other: 'Polytope', tol: float = 1e-8, device: int = 0) -> bool:
        """Whether ``other`` lies in this polytope: h_other(n_k) <= o_k + tol for every unit row [o_k | n_k] of this one
        (geometry.support.containment).  False for an ``other`` that is thin or unbounded where this polytope is bounded."""
        from .support import polytope_contains
        return polytope_contains(self, other, tol=tol, device=device)
