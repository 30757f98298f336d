"""The inputs the invariant-set tests share: the hand cases, worked out in the docstrings, and the seeded synthetic sets of
exit_cases.py.  No device and no package code: numpy only."""
import numpy

import exit_cases as xc

TOL = 1e-8
MAX_STEPS = 4          # of the synthetic sets

# (n_theta, seed, polytopes, varying coordinates, half-widths) of exit_cases.synthetic_set, the sizes of exit_cases.SETS.  The seeds were
# chosen on the CPU so that the share of knife items in the reference (invariant_reference.backward_reference, max_steps = 4) stays under KNIFE_CAP; the counts
# per seed are recorded in DESIGN §3.23 and asserted again by tests/test_invariant_set_cpu.py (the first set) and by the GPU file.
SETS = [(2, 6, 12, 2, (0.25, 0.45)), (3, 4, 24, 3, (0.12, 0.25)), (5, 23, 40, 5, (0.1, 0.18))]
KNIFE_CAP = 0.02


def predecessors_of(successors):
    """the predecessor lists of successor lists, ascending"""
    pred = [[] for _ in successors]
    for i, s in enumerate(successors):
        for j in sorted(set(int(v) for v in s)):
            pred[j].append(i)
    return pred


def one_d_cells0():
    """exit_cases.one_d_loop(4): the exit pieces by hand, in the order of ExitSets (by region L, M, U; M's pieces in the order
    of the cutting rows): L whole, M on [3/16, 1/4] and on [-1/4, -3/16], U whole.  M -> L, M, U are the only edges, so M is the one predecessor of each region.

    Step 1 pulls the four cells back through theta+ = 4 theta on M: [-3/16, -1/16] (from L), [3/64, 1/16] and [-1/16, -3/64] (from M's
    two cells) and [1/16, 3/16] (from U), in that order: per side the two cells tile [3/64, 3/16] = [0.1875 / 4, 0.1875].  Every later
    step divides by 4 again: step k >= 1 has, per side, a LARGE cell [1/16, 3/16] / 4^(k-1) of radius (1/16) / 4^(k-1) and a SMALL cell
    [3/64, 1/16] / 4^(k-1) of radius (1/128) / 4^(k-1), which tile [0.1875 / 4^k, 0.1875 / 4^(k-1)].  A cell is reported while its radius
    exceeds tol, so the small cells end first and the iteration converges after the last step whose large cell has a radius above tol."""
    return [(0, xc.box_rows([-0.75], [-0.25])), (1, xc.box_rows([0.1875], [0.25])), (1, xc.box_rows([-0.25], [-0.1875])),
            (2, xc.box_rows([0.25], [0.75]))]


def one_d_steps(tol):
    """(steps, last step with small cells) of the 1-D hand case: the last k >= 1 with (1/16) / 4^(k-1) > tol, and with (1/128) / 4^(k-1) > tol"""
    last = lambda r: max(k for k in range(1, 200) if r / 4.0 ** (k - 1) > tol)
    return last(1.0 / 16.0), last(1.0 / 128.0)


def rotation_grid():
    """The 4 x 4 grid of [-1, 1]^2, cell 4 r + c = [-1 + c / 2, -1 / 2 + c / 2] x [-1 + r / 2, -1 / 2 + r / 2], every cell with the map
    theta+ = 0.9 Rot(45 deg) theta.  The image leaves the box iff 0.9 max(|t1 - t2|, |t1 + t2|) / sqrt 2 > 1, i.e. |t1| + |t2| > s with
    s = sqrt 2 / 0.9 = 1.5713: E_0 is the four corner triangles of legs 2 - s = 0.4287 < 1/2, one inside each corner cell (cells 0, 3, 12,
    15), of area (2 - s)^2 / 2 each (the region difference may hand a triangle back in two pieces, split along the preimage of a grid
    line).  A state whose image lies in the triangle at (1, 1) has an image of norm >= s / sqrt 2 and of angle
    within [atan(s - 1), 90 deg - atan(s - 1)] = [29.7, 60.3] deg, so its own norm is >= s / (0.9 sqrt 2) = 1.2346 and its angle within
    +-15.3 deg: its first coordinate is >= 1.2346 cos 15.3 deg = 1.19 > 1, outside the box; by symmetry step 1 is empty and the iteration
    converges with steps = 0.  Invariant share: (4 - 2 (2 - s)^2) / 4.  Returns (polys, Phi, phi, successors): every pair is a candidate."""
    polys = [xc.box_rows([-1 + c / 2, -1 + r / 2], [-0.5 + c / 2, -0.5 + r / 2]) for r in range(4) for c in range(4)]
    a = 0.9 / numpy.sqrt(2.0)
    Phi = numpy.tile(numpy.array([[a, -a], [a, a]]), (16, 1, 1))
    return polys, Phi, numpy.zeros((16, 2)), [list(range(16)) for _ in range(16)]


ROTATION_SHARE = (4.0 - 2.0 * (2.0 - numpy.sqrt(2.0) / 0.9) ** 2) / 4.0


def straddle(m_i, m_q, seed=5):
    """One region of m_i rows and one cell of m_q rows in the plane (m_i + m_q straddles the words of the kept mask): the region is the
    square [-1, 1]^2 followed by m_i - 4 tangents of the circle of radius 2 (all redundant), with the map theta+ = theta / 2 + (1/4, 0);
    the cell is the half plane x >= 1/2 as its first row, then m_q - 1 tangents of the circle of radius 3 (redundant).  The new cell is
    {theta in the square : theta_1 / 2 + 1/4 >= 1/2} = [1/2, 1] x [-1, 1]: it keeps the rows x <= 1, y <= 1, y >= -1 of the square (bits
    0, 1, 3) and the pulled-back first row of the cell (bit m_i), four rows, whatever m_i and m_q.  Returns (polys, Phi, phi, cells0) with
    the region its own predecessor."""
    rng = numpy.random.default_rng(seed)
    ang = rng.uniform(0.0, 2.0 * numpy.pi, m_i - 4)
    region = numpy.vstack([xc.box_rows([-1, -1], [1, 1]), numpy.column_stack([numpy.full(m_i - 4, 2.0), numpy.cos(ang), numpy.sin(ang)])])
    ang = rng.uniform(0.0, 2.0 * numpy.pi, m_q - 1)
    cell = numpy.vstack([[[-0.5, -1.0, 0.0]], numpy.column_stack([numpy.full(m_q - 1, 3.0), numpy.cos(ang), numpy.sin(ang)])])
    return [region], numpy.array([[[0.5, 0.0], [0.0, 0.5]]]), numpy.array([[0.25, 0.0]]), [(0, cell)]
