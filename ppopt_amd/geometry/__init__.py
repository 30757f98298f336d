"""Polytopes of parameter space and uniform sampling in them (reference: geometry/)."""
from .polytope import Polytope
from .polytope_operations import (DEFAULT_N_STEPS, find_extents, get_chebyshev_information, hit_and_run, hit_and_run_batch,
                                  sample_program_theta_space)
from .reduce import ReducedRows, reduce_polytopes, reduce_rows_of
from .project import ProjectedRows, affine_image, controllable_pre, minkowski_sum, project_polytopes, project_rows_of
from .support import (Containment, ErodedRows, OutputRange, SupportValues, containment, pontryagin_difference, robust_controllable_pre,
                      support, support_of)
from .slice import LineSlice, SolutionSlice, slice_polytopes
from .moments import ExpectedValues, RegionMoments, integrate_quadratic, moments_of_rows, polytope_moments
from .box_pairs import box_pairs, screen_pairs
from .volume import CoverageVolume, RegionVolumes, polytope_volumes, volumes_of_rows
