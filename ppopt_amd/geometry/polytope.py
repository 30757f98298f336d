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
