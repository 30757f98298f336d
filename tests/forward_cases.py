"""The inputs the forward-cell tests share: the hand cases, worked out in the docstrings, the seeded synthetic sets of
exit_cases.py and the sheared grid partitions.  No device and no package code: numpy only."""
import itertools

import numpy

import exit_cases as xc

TOL = 1e-8
SET_TOL = 1e-6         # of the synthetic sets and the sheared grids
SET_STEPS = 3

# exit_cases.SETS, as the issue lists them: (n_theta, seed, polytopes, varying coordinates, half-widths).  Knife items of the reference
# (forward_reference.forward_reference, step 0 = the polytopes, successors from the reference graph, 3 steps, tol = 1e-6), counted on the
# CPU: recorded in DESIGN §3.25 and asserted again by the GPU file; the cap is 2 % of a case's items.
SETS = list(xc.SETS)
KNIFE_CAP = 0.02

# (n_theta, boxes per axis, seed, steps) of sheared_grid for the point tests; the seeds were chosen with the reference alone on the CPU
GRIDS = [(2, 4, 2, 4), (3, 3, 2, 3)]


def tent_map():
    """R_0 = [0, 1/2] with theta+ = 2 theta and R_1 = [1/2, 1] with theta+ = 2 - 2 theta: both images are [0, 1], so every region follows
    every region.  Rows and maps are exact in binary.  Returns (polys, Phi, phi, successors)."""
    polys = [xc.box_rows([0.0], [0.5]), xc.box_rows([0.5], [1.0])]
    return polys, numpy.array([[[2.0]], [[-2.0]]]), numpy.array([[0.0], [2.0]]), [[0, 1], [0, 1]]


def tent_cells(steps):
    """The cells of the tent map by hand, step by step in item order: [(lo, hi, G, g, region, parent)].  A cell Q = [a, b] of step k with
    region i is mapped ONTO [0, 1] by its next map P = Phi_i G, s = Phi_i g + phi_i (|P| = 2^(k + 1), b - a = 2^-(k + 1)); with m the
    midpoint, the child of region 0 (image in [0, 1/2]) is [a, m] when P > 0 and [m, b] when P < 0, the child of region 1 the other half.
    Step k has 2^(k + 1) cells: the dyadic intervals of length 2^-(k + 1).  Every number is a dyadic rational far inside the 53 bits, so
    the float arithmetic below is exact."""
    Phi, phi = (2.0, -2.0), (0.0, 2.0)
    cells = [(0.0, 0.5, 1.0, 0.0, 0, -1), (0.5, 1.0, 1.0, 0.0, 1, -1)]
    lo, hi = 0, 2
    for _ in range(steps):
        for c in range(lo, hi):
            a, b, G, g, i, _p = cells[c]
            P, s = Phi[i] * G, Phi[i] * g + phi[i]
            m = 0.5 * (a + b)
            for j in (0, 1):
                low_half = (P > 0) == (j == 0)
                cells.append((a, m, P, s, j, c) if low_half else (m, b, P, s, j, c))
        lo, hi = hi, len(cells)
    return cells


def tent_rows(cell):
    """The two rows a tent cell of a step >= 1 keeps, by hand: the rows x <= hi_j and -x <= -lo_j of its region R_j pulled back through
    its own map (G, g): [(hi_j - g) / |G|, sign G] and [(g - lo_j) / |G|, -sign G], in the order of R_j's rows.  The rows of the parent
    are met first by the row loop and are redundant beside these (the pulled-back set lies inside the parent)."""
    _, _, G, g, j, _ = cell
    lo_j, hi_j = (0.0, 0.5) if j == 0 else (0.5, 1.0)
    sgn = 1.0 if G > 0 else -1.0
    return numpy.array([[(hi_j - g) / abs(G), sgn], [(g - lo_j) / abs(G), -sgn]])


def sheared_grid(n, g, seed):
    """The g^n boxes of [-1, 1]^n under one seeded linear map M = I + 0.3 N(0, 1): a partition of M [-1, 1]^n into g^n parallelepipeds
    that do not overlap (box k = the mixed-radix digits of k, first coordinate slowest).  The box {lo <= z <= hi} becomes
    {theta : lo <= M^-1 theta <= hi}: the rows (M^-T e_t) theta <= hi_t and -(M^-T e_t) theta <= -lo_t, scaled to unit normals.  The maps
    go round exit_cases.KINDS (contraction, rotation, rank-deficient, zero, shifted identity).  Every region may follow every region.
    Returns (polys, Phi, phi, successors, M)."""
    rng = numpy.random.default_rng(seed)
    M = numpy.eye(n) + 0.3 * rng.normal(size=(n, n))
    W = numpy.linalg.inv(M)                       # z = W theta
    edges = numpy.linspace(-1.0, 1.0, g + 1)
    polys, Phi, phi = [], [], []
    for q, digits in enumerate(itertools.product(range(g), repeat=n)):
        lo, hi = edges[list(digits)], edges[[d + 1 for d in digits]]
        rows = numpy.vstack([numpy.column_stack([hi, W]), numpy.column_stack([-lo, -W])])
        polys.append(rows / numpy.linalg.norm(rows[:, 1:], axis=1, keepdims=True))
        P, p = xc._map(xc.KINDS[q % len(xc.KINDS)], n, n, rng)
        Phi.append(P)
        phi.append(p)
    R = len(polys)
    return polys, numpy.asarray(Phi), numpy.asarray(phi), [list(range(R)) for _ in range(R)], M


def grid_points(M, n_points, seed):
    """n_points uniform points of X_0 = M [-1, 1]^n"""
    rng = numpy.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (n_points, len(M))) @ M.T


def polygon(n, shift=0.0):
    """the regular n-gon around the unit circle as unit rows, turned by ``shift`` sides"""
    ang = 2.0 * numpy.pi * (numpy.arange(n) + shift) / n
    return numpy.column_stack([numpy.ones(n), numpy.cos(ang), numpy.sin(ang)])
