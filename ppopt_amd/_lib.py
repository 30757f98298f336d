"""ctypes binding of libmpcombi_hip.so (the C ABI declared in include/mpcombi.h).

This is the only doorway from the Python host code to the device kernels.  There is no CPU fallback: if the
shared library is missing, or no HIP device is usable, every call raises ``MpcError``.
"""
import ctypes
import weakref
import os
from typing import Optional

import numpy

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MPC_LIB_PATH') or os.path.join(_HERE, 'csrc', 'libmpcombi_hip.so')   # MPC_LIB_PATH: A/B builds

MPC_OK, MPC_ERR_INVALID, MPC_ERR_HIP, MPC_ERR_CAPACITY, MPC_ERR_STATE = range(5)
MPC_LOCATE_OVERLAPPING, MPC_LOCATE_INCLUSIVE, MPC_LOCATE_WALK, MPC_LOCATE_TREE = 1, 2, 4, 8   # flags of mpc_locator_query
MPC_SIM_FINAL, MPC_SIM_KEY_SALT = 16, 0x636c6f6f   # flag of mpc_locator_simulate (record the final states only); its Philox key salt
SIM_MAX_DIM, SIM_MAX_INPUTS, SIM_DEFAULT_BUDGET = 16, 16, 4 << 30   # limits of mpc_locator_simulate
VX_OK, VX_UNBOUNDED, VX_NOT_POINTED, VX_EMPTY, VX_OVERFLOW = range(5)   # statuses of mpc_region_vertices
VX_MAX_DIM, VX_MAX_ROWS, VX_DEFAULT_BUDGET, VX_DEFAULT_SLAB, VX_MAX_SLAB = 16, 256, 4 << 30, 256, 1 << 24   # its limits
VOL_OK, VOL_UNBOUNDED, VOL_NOT_POINTED, VOL_EMPTY, VOL_OVERFLOW, VOL_TOO_LARGE, VOL_INCONSISTENT = range(7)   # statuses of mpc_region_volumes
VOL_MAX_VERTS, VOL_DEFAULT_BUDGET, VOL_DEFAULT_MAX_SIMPLICES = 16384, 4 << 30, 1 << 16   # its limits and the default work cap
TREE_MAX_DIM, TREE_MAX_ROWS, TREE_MAX_DEPTH = 16, 256, 64   # limits of mpc_tree_build
MPC_SOLVE_MANY_BASE = 128   # flag of mpc_solve_many_start
MPC_LEVEL_STREAM, MPC_LEVEL_GRAPH, MPC_LEVEL_THEN_BASE, MPC_LEVEL_KEEP_LOWDIM, MPC_LEVEL_ONLY_BASE = 1, 4, 8, 16, 32   # flags of mpc_level_start / mpc_level_run_ex
MPC_SOLVE_FETCH = 64   # flag of mpc_solve_start
MPC_HR_OK, MPC_HR_OUTSIDE, MPC_HR_UNBOUNDED = range(3)   # chain statuses of mpc_hit_and_run
HR_MAX_DIM, HR_MAX_ROWS = 64, 256   # limits of mpc_hit_and_run
MPC_SLICE_FULL, MPC_SLICE_EMPTY, MPC_SLICE_LOWDIM, MPC_SLICE_CUT = 0, 1, 2, 4   # statuses of mpc_slice_polygons / _intervals (CUT: a flag)
SLICE_EPS = 1e-9   # default of the one tolerance argument of the slice kernels
INFEASIBLE, FEASIBLE, OPTIMAL_NO_REGION, REGION, SINGULAR_KKT, LP_LIMIT = range(6)
LP_OPTIMAL, LP_INFEASIBLE, LP_UNBOUNDED, LP_ITERLIMIT = range(4)
MASK_WORDS = 2

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_lp = ctypes.POINTER(ctypes.c_int64)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_u64p = ctypes.POINTER(ctypes.c_uint64)


class MpcError(RuntimeError):
    code = 0


class MpcCapacityError(MpcError):
    """MPC_ERR_CAPACITY from a level: the overlapped region stage found more late optimal candidates than it had reserved
    slots for (mpcombi.h, mpc_set_region_overlap).  The drivers repeat the solve with the overlap switched off."""
    code = 3


class MpcProblem(ctypes.Structure):
    _fields_ = [('n_x', ctypes.c_int32), ('n_t', ctypes.c_int32), ('n_c', ctypes.c_int32), ('n_eq', ctypes.c_int32),
                ('n_tc', ctypes.c_int32), ('A', _dp), ('b', _dp), ('F', _dp), ('c', _dp), ('H', _dp), ('Q', _dp),
                ('A_t', _dp), ('b_t', _dp)]


class LevelStats(ctypes.Structure):
    _fields_ = [('n', ctypes.c_int64), ('k', ctypes.c_int32), ('kkt_mode', ctypes.c_int32),
                ('n_status', ctypes.c_int64 * 6), ('n_regions', ctypes.c_int64), ('n_children', ctypes.c_int64),
                ('n_pruned_new', ctypes.c_int64), ('lp_pivots', ctypes.c_int64), ('ms_verdict', ctypes.c_float),
                ('ms_region', ctypes.c_float), ('ms_children', ctypes.c_float), ('ms_total', ctypes.c_float),
                ('n_xtheta_lp', ctypes.c_int64), ('n_xtheta_fallback', ctypes.c_int64),
                ('wave_cycles', ctypes.c_int64 * 4), ('n_region_retry', ctypes.c_int64),
                ('n_x_cached', ctypes.c_int64), ('ms_theta', ctypes.c_float), ('ms_x', ctypes.c_float),
                ('ms_region2', ctypes.c_float), ('region_side_stream', ctypes.c_float), ('n_x_items', ctypes.c_int64),
                ('n_opt', ctypes.c_int64), ('dict_read_bytes', ctypes.c_int64), ('dict_write_bytes', ctypes.c_int64),
                ('n_theta_items', ctypes.c_int64), ('n_region_rows', ctypes.c_int64),
                ('ms_kkt', ctypes.c_float), ('ms_xq', ctypes.c_float), ('n_xq_items', ctypes.c_int64), ('xq_pivots', ctypes.c_int64),
                ('xq_record_ints', ctypes.c_int64), ('xq_record_rows', ctypes.c_int64), ('xq_record_cols', ctypes.c_int64),
                ('n_xq_thread', ctypes.c_int64), ('ms_xq_thread', ctypes.c_float), ('xq_thread_beside_theta', ctypes.c_float),
                ('n_x1', ctypes.c_int64), ('ms_x1', ctypes.c_float), ('ms_x_plan', ctypes.c_float)]


class SolveLevelInfo(ctypes.Structure):
    """mpc_solve_level_info (include/mpcombi.h)."""
    _fields_ = [('level', ctypes.c_int32), ('k', ctypes.c_int32), ('mode', ctypes.c_int32), ('chunk', ctypes.c_int32),
                ('n_chunks', ctypes.c_int32), ('pad_', ctypes.c_int32), ('n', ctypes.c_int64), ('n_slots', ctypes.c_int64),
                ('n_rows', ctypes.c_int64), ('head_d', ctypes.c_void_p), ('head_i', ctypes.c_void_p), ('erows', ctypes.c_void_p)]


class ManyLevelInfo(ctypes.Structure):
    """mpc_many_level_info (include/mpcombi.h)."""
    _fields_ = [('level', ctypes.c_int32), ('n_members', ctypes.c_int32), ('n_shared', ctypes.c_int32), ('done', ctypes.c_int32),
                ('base', ctypes.c_int32), ('pad_', ctypes.c_int32),
                ('member', ctypes.POINTER(ctypes.c_int32)), ('stats', ctypes.POINTER(LevelStats)),
                ('n_slots', ctypes.POINTER(ctypes.c_int64)), ('n_rows', ctypes.POINTER(ctypes.c_int64)),
                ('off_d', ctypes.POINTER(ctypes.c_int64)), ('off_i', ctypes.POINTER(ctypes.c_int64)), ('off_e', ctypes.POINTER(ctypes.c_int64)),
                ('head_d', ctypes.c_void_p), ('head_i', ctypes.c_void_p), ('erows', ctypes.c_void_p),
                ('len_d', ctypes.c_int64), ('len_i', ctypes.c_int64), ('len_e', ctypes.c_int64), ('ms_wall', ctypes.c_double)]


_lib = None


def _share_the_hip_runtime_with_torch():
    """PyTorch-ROCm wheels carry their own libamdhip64.so.  Two HIP runtimes in one process cannot both open the GPU: when this
    library (linked against /opt/rocm's runtime) is loaded BEFORE torch, a later ``torch.cuda`` call fails with "No HIP GPUs are
    available".  If torch is installed but not imported yet, its runtime is loaded here first, globally, so that this library and
    torch bind to the same one -- the state a process is in anyway when torch was imported first.  ``MPC_NO_TORCH_HIP=1`` skips it."""
    import sys
    if 'torch' in sys.modules or os.environ.get('MPC_NO_TORCH_HIP', '0') == '1':
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec('torch')
        if spec is None or not spec.origin:
            return
        path = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so')
        if os.path.exists(path):
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    except Exception:       # no torch, or an unusual layout: the library's own runtime is used
        pass


class TreeStats(ctypes.Structure):
    """mpc_tree_stats (include/mpcombi.h)"""
    _fields_ = [(n, ctypes.c_int64) for n in ('n_nodes', 'n_leaves', 'depth', 'max_leaf', 'leaf_items')] + [('mean_leaf', ctypes.c_double)] + \
               [(n, ctypes.c_int64) for n in ('pairs', 'box_pairs', 'lps', 'pivots', 'capped', 'tau_lps', 'bitset_bytes')] + \
               [(n, ctypes.c_double) for n in ('ms_classify', 'ms_split', 'ms_tau', 'ms_total')]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class SimStats(ctypes.Structure):
    """mpc_sim_stats (include/mpcombi.h)"""
    _fields_ = [('traj_steps', ctypes.c_int64), ('crossings', ctypes.c_int64), ('fallbacks', ctypes.c_int64), ('mode', ctypes.c_int32),
                ('ms', ctypes.c_float)]


class VertexStats(ctypes.Structure):
    """mpc_vertex_stats (include/mpcombi.h)"""
    _fields_ = [('generators', ctypes.c_int64), ('max_list', ctypes.c_int64), ('merges', ctypes.c_int64), ('repeats', ctypes.c_int64),
                ('overflow', ctypes.c_int64), ('launches', ctypes.c_int64), ('slab', ctypes.c_int64), ('ms', ctypes.c_float)]


class VolumeStats(ctypes.Structure):
    """mpc_volume_stats (include/mpcombi.h)"""
    _fields_ = [('simplices', ctypes.c_int64), ('max_simplices', ctypes.c_int64), ('launches', ctypes.c_int64),
                ('status_counts', ctypes.c_int64 * 7), ('ms', ctypes.c_float)]


def load():
    """Loads the HIP library; raises MpcError (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MpcError(f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                       f'(hipcc --offload-arch=gfx950). ppopt_amd has no CPU fallback.')
    _share_the_hip_runtime_with_torch()
    L = ctypes.CDLL(LIB_PATH)
    H = ctypes.c_void_p
    sig = {
        'mpc_device_count': (ctypes.c_int, []),
        'mpc_version': (ctypes.c_char_p, []),
        'mpc_last_global_error': (ctypes.c_char_p, []),
        'mpc_create': (ctypes.c_int, [ctypes.POINTER(MpcProblem), ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(H)]),
        'mpc_destroy': (ctypes.c_int, [H]),
        'mpc_last_error': (ctypes.c_char_p, [H]),
        'mpc_mask_words': (ctypes.c_int32, [H]),
        'mpc_set_region_overlap': (ctypes.c_int, [H, ctypes.c_int32]),
        'mpc_set_timing': (ctypes.c_int, [H, ctypes.c_int32]),
        'mpc_engine_kind': (ctypes.c_int, [H, ctypes.POINTER(ctypes.c_int32)]),
        'mpc_program_block': (ctypes.c_int, [H, ctypes.c_int32, _dp, ctypes.c_int64, _lp]),
        'mpc_region_doubles': (ctypes.c_int64, [H]),
        'mpc_region_ints': (ctypes.c_int64, [H]),
        'mpc_lds_bytes': (ctypes.c_int32, [H, ctypes.c_int32]),
        'mpc_stream': (ctypes.c_void_p, [H]),
        'mpc_frontier_root': (ctypes.c_int, [H]),
        'mpc_frontier_set': (ctypes.c_int, [H, _ip, ctypes.c_int64, ctypes.c_int32]),
        'mpc_frontier_set_device': (ctypes.c_int, [H, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32]),
        'mpc_frontier_info': (ctypes.c_int, [H, _lp, _ip]),
        'mpc_frontier_get': (ctypes.c_int, [H, _ip, ctypes.c_int64]),
        'mpc_pruned_clear': (ctypes.c_int, [H]),
        'mpc_pruned_add': (ctypes.c_int, [H, _u64p, ctypes.c_int64]),
        'mpc_pruned_add_device': (ctypes.c_int, [H, ctypes.c_void_p, ctypes.c_int64]),
        'mpc_pruned_count': (ctypes.c_int64, [H]),
        'mpc_pruned_get': (ctypes.c_int, [H, _u64p, ctypes.c_int64]),
        'mpc_level_run': (ctypes.c_int, [H, ctypes.c_int32, ctypes.POINTER(LevelStats)]),
        'mpc_level_run_ex': (ctypes.c_int, [H, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(LevelStats)]),
        'mpc_level_run_batch': (ctypes.c_int, [ctypes.POINTER(H), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.POINTER(LevelStats), ctypes.POINTER(ctypes.c_int32)]),
        'mpc_level_batch_start': (ctypes.c_int, [ctypes.POINTER(H), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]),
        'mpc_level_batch_wait': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(LevelStats), ctypes.POINTER(ctypes.c_int32)]),
        'mpc_level_memory_gb': (ctypes.c_double, [H, ctypes.c_int32]),
        'mpc_frontier_advance_batch': (ctypes.c_int, [ctypes.POINTER(H), ctypes.c_int32]),
        'mpc_trim': (ctypes.c_int, [H]),
        'mpc_level_status': (ctypes.c_int, [H, _u8p]),
        'mpc_level_start': (ctypes.c_int, [H, ctypes.c_int32, ctypes.c_int32]),
        'mpc_level_stream_info': (ctypes.c_int, [H, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                                 ctypes.POINTER(ctypes.c_void_p), _lp, _lp, _ip, _ip]),
        'mpc_level_chunk_wait': (ctypes.c_int, [H, ctypes.c_int32]),
        'mpc_level_wait': (ctypes.c_int, [H, ctypes.POINTER(LevelStats)]),
        'mpc_level_stream_fixup': (ctypes.c_int, [H, _dp, _ip, _dp, _lp]),
        'mpc_base_result': (ctypes.c_int, [H, _u8p, _lp, _dp, _ip]),
        'mpc_solve_start': (ctypes.c_int, [H, ctypes.c_int32, ctypes.c_int32]),
        'mpc_solve_level': (ctypes.c_int, [H, ctypes.c_int32, ctypes.POINTER(SolveLevelInfo)]),
        'mpc_solve_chunk_wait': (ctypes.c_int, [H, ctypes.c_int32, ctypes.c_int32]),
        'mpc_solve_level_wait': (ctypes.c_int, [H, ctypes.c_int32, ctypes.POINTER(LevelStats), ctypes.POINTER(ctypes.c_double)]),
        'mpc_solve_wait': (ctypes.c_int, [H, ctypes.POINTER(ctypes.c_int32)]),
        'mpc_level_regions': (ctypes.c_int, [H, _dp, _ip, _lp, ctypes.c_int64]),
        'mpc_compact_strides': (ctypes.c_int, [H, _lp, _lp, _lp]),
        'mpc_level_regions_compact': (ctypes.c_int, [H, _dp, _ip, ctypes.c_int64, _dp, ctypes.c_int64, _lp, _lp]),
        'mpc_frontier_shard': (ctypes.c_int, [H, ctypes.c_int32, ctypes.c_int32]),
        'mpc_level_slots': (ctypes.c_int64, [H]),
        'mpc_level_regions_slots': (ctypes.c_int, [H, _dp, _ip, ctypes.c_int64, _dp, ctypes.c_int64, _lp, _lp]),
        'mpc_level_regions_slots_async': (ctypes.c_int, [H, _dp, _ip, ctypes.c_int64, _dp, ctypes.c_int64, _lp, _lp]),
        'mpc_level_regions_slots_nowait': (ctypes.c_int, [H, _dp, _ip, ctypes.c_int64, _dp, ctypes.c_int64, _lp, _lp]),
        'mpc_level_batch_fetch': (ctypes.c_int, [ctypes.POINTER(H), ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), _lp, ctypes.POINTER(ctypes.c_void_p), _lp, _lp, _lp]),
        'mpc_sync': (ctypes.c_int, [H]),
        'mpc_fetch_wait': (ctypes.c_int, [ctypes.c_int32]),
        'mpc_solve_many_start': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]),
        'mpc_solve_many_level': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ManyLevelInfo)]),
        'mpc_solve_many_wait': (ctypes.c_int, [ctypes.c_void_p]),
        'mpc_locator_create': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, _dp, _dp, _dp,
                                               ctypes.POINTER(ctypes.c_void_p)]),
        'mpc_locator_query': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, _dp, ctypes.c_double, ctypes.c_int32, _lp, _dp,
                                              ctypes.POINTER(ctypes.c_float)]),
        'mpc_locator_last_unresolved': (ctypes.c_int, [ctypes.c_void_p, _lp]),
        'mpc_locator_destroy': (ctypes.c_int, [ctypes.c_void_p]),
        'mpc_locator_set_adjacency': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, _u64p, _ip]),
        'mpc_host_alloc': (ctypes.c_int, [ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]),
        'mpc_host_free': (ctypes.c_int, [ctypes.c_void_p]),
        'mpc_level_children': (ctypes.c_int, [H, _ip, ctypes.c_int64]),
        'mpc_level_children_device': (ctypes.c_int, [H, ctypes.c_void_p, ctypes.c_int64]),
        'mpc_level_pruned_new': (ctypes.c_int, [H, _u64p, ctypes.c_int64]),
        'mpc_level_pruned_new_device': (ctypes.c_int, [H, ctypes.c_void_p, ctypes.c_int64]),
        'mpc_level_regions_device': (ctypes.c_int, [H, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                    ctypes.c_int64, _lp, _lp]),
        'mpc_frontier_advance': (ctypes.c_int, [H]),
        'mpc_qp_solve_batch': (ctypes.c_int, [H, ctypes.c_int64, _dp, _ip, _dp, _dp, _u8p, _ip]),
        'mpc_facet_centres': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, _dp, _ip]),
        'mpc_graph_begin': (ctypes.c_int, [H, _u64p, ctypes.c_int64, ctypes.c_int32]),
        'mpc_graph_wave': (ctypes.c_int, [H, _ip, _lp, ctypes.c_int32, _ip, _lp, _lp]),
        'mpc_graph_group_run': (ctypes.c_int, [H, ctypes.c_int32, ctypes.POINTER(LevelStats)]),
        'mpc_graph_wave_close': (ctypes.c_int, [H, _lp, _lp]),
        'mpc_check_level': (ctypes.c_int, [H, _ip, ctypes.c_int64, ctypes.c_int32, _u64p, ctypes.c_int64, ctypes.c_int32,
                                           _u8p, _lp, _dp, _ip, _lp, ctypes.c_int64, _lp, _ip, ctypes.c_int64]),
        'mpc_lp_solve_batch': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _dp,
                                              ctypes.c_int32, _dp, ctypes.c_int32, _dp, ctypes.c_int32, _u8p, _ip, _dp,
                                              _dp, _ip]),
        'mpc_miqp_solve_batch': (ctypes.c_int, [ctypes.c_int32] + [ctypes.c_int32] * 5 + [_dp] * 7 + [ctypes.c_int32, _dp, _u8p, _ip,
                                                ctypes.c_int32, _ip, ctypes.c_int64, _dp, ctypes.c_int64, _dp, _ip, _ip, _dp, _dp,
                                                _dp, _u8p]),
        'mpc_hit_and_run': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_int64, ctypes.c_uint64, _dp, _ip, ctypes.POINTER(ctypes.c_float)]),
        'mpc_slice_polygons': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, _dp, _dp, ctypes.c_double,
                                              _dp, _ip, _ip, _dp, _ip, ctypes.POINTER(ctypes.c_float)]),
        'mpc_slice_intervals': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, _dp, ctypes.c_double,
                                               ctypes.c_double, ctypes.c_double, _dp, _ip, ctypes.POINTER(ctypes.c_float)]),
        'mpc_tree_build': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _dp, _lp, _ip, ctypes.c_double, ctypes.c_double, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(TreeStats)]),
        'mpc_locator_tree_size': (ctypes.c_int, [ctypes.c_void_p, _lp, _lp, _ip, _dp]),
        'mpc_locator_get_tree': (ctypes.c_int, [ctypes.c_void_p, _dp, _ip, _ip, _dp, _lp, _ip]),
        'mpc_locator_set_tree': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _dp, ctypes.c_int64, _ip, _ip, _dp, _lp, _ip, ctypes.c_double]),
        'mpc_locator_simulate': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _dp, ctypes.c_int32, _ip, _dp, _dp, _dp, _dp, _dp,
                                                 _dp, ctypes.c_uint64, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_int64, _dp, _dp,
                                                 _ip, _ip, _ip, ctypes.POINTER(SimStats)]),
        'mpc_region_vertices': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, ctypes.c_double, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.c_int64, _lp, _lp, _ip, _lp, _lp, _dp, ctypes.POINTER(ctypes.c_uint64), _dp,
                                                ctypes.POINTER(VertexStats)]),
        'mpc_region_volumes': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _lp, _dp, ctypes.POINTER(ctypes.c_uint64), _ip,
                                               ctypes.c_double, ctypes.c_int64, ctypes.c_int64, _dp, _dp, _lp, _ip, ctypes.POINTER(VolumeStats)]),
        'mpc_region_moments': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _lp, _dp, ctypes.POINTER(ctypes.c_uint64), _ip,
                                               ctypes.c_double, ctypes.c_int64, ctypes.c_int64, _dp, _dp, _lp, _ip, _dp, ctypes.POINTER(VolumeStats)]),
        'mpc_merge_regions': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, _dp, _ip, _lp,
                                             ctypes.POINTER(ctypes.c_float)]),
        'mpc_merge_pairs': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, _dp, ctypes.c_int64, _ip, _ip,
                                           ctypes.c_double, _u64p, _u64p, _ip, _dp, _lp, ctypes.POINTER(ctypes.c_float)]),
        'mpc_overlap_pairs': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, ctypes.c_int64, _ip, _ip, _ip, _dp,
                                             ctypes.c_double, _dp, _dp, _dp, _ip, _lp, ctypes.POINTER(ctypes.c_float)]),
        'mpc_law_gap_pairs': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, _dp, ctypes.c_int64, _ip,
                                             _ip, ctypes.c_double, _dp, _dp, _ip, _dp, _dp, _ip, _lp, ctypes.POINTER(ctypes.c_float)]),
        'mpc_box_pairs': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _dp, _u8p, ctypes.c_int64, _dp, _u8p,
                                         ctypes.c_double, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _lp, _lp, _lp, _lp, _lp,
                                         ctypes.POINTER(ctypes.c_float)]),
        'mpc_pair_screen': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, ctypes.c_int64, _lp, _lp, _dp, _dp,
                                           ctypes.c_int32, _u8p, _lp, ctypes.POINTER(ctypes.c_float)]),
        'mpc_overlap_split': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, ctypes.c_int64, _lp, _dp, ctypes.c_int64,
                                             _ip, _ip, _ip, _dp, _dp, ctypes.c_double, _ip, _u64p, _lp, ctypes.POINTER(ctypes.c_float)]),
        'mpc_transition_boxes': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, _dp, _dp, _dp, _ip, _lp,
                                                ctypes.POINTER(ctypes.c_float)]),
        'mpc_transition_pairs': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, _dp, _dp, ctypes.c_int64, _ip, _ip,
                                                ctypes.c_int32, ctypes.c_double, _dp, _ip, _dp, _lp, ctypes.POINTER(ctypes.c_float)]),
        'mpc_exit_split': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, _dp, ctypes.c_int64, _lp, _dp, ctypes.c_int64,
                                          _ip, _ip, _ip, _dp, ctypes.c_double, _ip, _u64p, _lp, ctypes.POINTER(ctypes.c_float)]),
        'mpc_reduce_rows': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, ctypes.c_double, _ip, _ip, _u64p, _dp, _lp,
                                           ctypes.POINTER(ctypes.c_float)]),
        'mpc_support_rows': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _lp, _dp, _dp, ctypes.c_double, _dp, _dp, _ip,
                                            _ip, _ip, _dp, _lp, ctypes.POINTER(ctypes.c_float)]),
        'mpc_project_rows': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, ctypes.c_double,
                                            ctypes.c_int32, _dp, _ip, _ip, _ip, _ip, _dp, _lp, ctypes.POINTER(ctypes.c_float)]),
        'mpc_backward_exits': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, _dp, _dp, _lp, _ip, ctypes.c_int64, _lp, _dp,
                                              _ip, ctypes.c_double, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, _lp, _lp, _dp, _ip, _ip, _ip, _ip, _dp,
                                              _ip, _ip, _ip, _lp, ctypes.POINTER(ctypes.c_float), _lp, ctypes.POINTER(ctypes.c_float)]),
        'mpc_forward_cells': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _lp, _dp, _dp, _dp, _lp, _ip, ctypes.c_int64, _lp, _dp,
                                             _ip, _dp, ctypes.c_double, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, _lp, _lp, _dp, _ip, _ip, _ip, _ip,
                                             _dp, _dp, _ip, _ip, _lp, ctypes.POINTER(ctypes.c_float), _lp, ctypes.POINTER(ctypes.c_float)]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get('MPC_LIB_ALLOW_MISSING') == '1' and not hasattr(L, name):
            continue      # tools/ab_lib.py comparing against an OLDER build of the library (MPC_LIB_PATH); never set in tests
        fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


EXPORTED_SYMBOLS = ['mpc_device_count', 'mpc_version', 'mpc_last_global_error', 'mpc_create', 'mpc_destroy',
                    'mpc_last_error', 'mpc_mask_words', 'mpc_set_region_overlap', 'mpc_set_timing', 'mpc_engine_kind', 'mpc_program_block', 'mpc_region_doubles', 'mpc_region_ints', 'mpc_lds_bytes', 'mpc_stream',
                    'mpc_frontier_root', 'mpc_frontier_set', 'mpc_frontier_set_device', 'mpc_frontier_info',
                    'mpc_frontier_get', 'mpc_pruned_clear', 'mpc_pruned_add', 'mpc_pruned_add_device',
                    'mpc_pruned_count', 'mpc_pruned_get', 'mpc_level_run', 'mpc_level_run_ex', 'mpc_level_run_batch', 'mpc_frontier_advance_batch', 'mpc_level_memory_gb', 'mpc_trim', 'mpc_level_batch_start', 'mpc_level_batch_wait', 'mpc_level_regions_slots_nowait', 'mpc_level_batch_fetch', 'mpc_level_status', 'mpc_level_start', 'mpc_level_stream_info', 'mpc_level_chunk_wait', 'mpc_level_wait', 'mpc_level_stream_fixup', 'mpc_base_result', 'mpc_solve_start', 'mpc_solve_level', 'mpc_solve_chunk_wait', 'mpc_solve_level_wait', 'mpc_solve_wait', 'mpc_level_regions', 'mpc_compact_strides',
                    'mpc_level_regions_compact', 'mpc_frontier_shard', 'mpc_level_slots', 'mpc_level_regions_slots', 'mpc_level_regions_slots_async', 'mpc_sync', 'mpc_fetch_wait', 'mpc_solve_many_start', 'mpc_solve_many_level', 'mpc_solve_many_wait', 'mpc_host_alloc', 'mpc_host_free', 'mpc_locator_create', 'mpc_locator_query', 'mpc_locator_last_unresolved', 'mpc_locator_destroy', 'mpc_locator_set_adjacency', 'mpc_level_children', 'mpc_level_children_device', 'mpc_level_pruned_new',
                    'mpc_level_pruned_new_device', 'mpc_level_regions_device', 'mpc_frontier_advance', 'mpc_qp_solve_batch', 'mpc_facet_centres', 'mpc_graph_begin', 'mpc_graph_wave', 'mpc_graph_group_run', 'mpc_graph_wave_close', 'mpc_check_level', 'mpc_lp_solve_batch', 'mpc_miqp_solve_batch', 'mpc_hit_and_run', 'mpc_slice_polygons', 'mpc_slice_intervals',
                    'mpc_tree_build', 'mpc_locator_tree_size', 'mpc_locator_get_tree', 'mpc_locator_set_tree', 'mpc_merge_regions',
                    'mpc_merge_pairs', 'mpc_locator_simulate', 'mpc_region_vertices', 'mpc_region_volumes', 'mpc_region_moments',
                    'mpc_overlap_pairs', 'mpc_overlap_split', 'mpc_transition_boxes', 'mpc_transition_pairs', 'mpc_exit_split', 'mpc_reduce_rows',
                    'mpc_backward_exits', 'mpc_project_rows', 'mpc_forward_cells', 'mpc_law_gap_pairs', 'mpc_box_pairs',
                    'mpc_pair_screen', 'mpc_support_rows']


def pinned_empty(shape, dtype) -> numpy.ndarray:
    """An uninitialised array in pooled page-locked host memory (mpc_host_alloc); the block goes back to the pool when
    the last view of the array is gone."""
    L = load()
    dtype = numpy.dtype(dtype)
    count = int(numpy.prod(shape))
    nbytes = max(count * dtype.itemsize, 1)
    ptr = ctypes.c_void_p()
    if L.mpc_host_alloc(nbytes, ctypes.byref(ptr)) != 0:
        raise MemoryError(f'mpc_host_alloc({nbytes}) failed')
    buf = (ctypes.c_char * nbytes).from_address(ptr.value)
    weakref.finalize(buf, L.mpc_host_free, ctypes.c_void_p(ptr.value))
    return numpy.frombuffer(buf, dtype=dtype, count=count).reshape(shape)


def pinned_adopt(ptr: int, shape, dtype) -> numpy.ndarray:
    """An array over a page-locked block the library has handed over (mpc_level_stream_info): same ownership rule as
    pinned_empty -- the block returns to the pool with the last view."""
    L = load()
    dtype = numpy.dtype(dtype)
    count = int(numpy.prod(shape))
    nbytes = max(count * dtype.itemsize, 1)
    buf = (ctypes.c_char * nbytes).from_address(ptr)
    weakref.finalize(buf, L.mpc_host_free, ctypes.c_void_p(ptr))
    return numpy.frombuffer(buf, dtype=dtype, count=count).reshape(shape)


def _f64(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64)


def sets_to_masks(sets, words: int = MASK_WORDS) -> numpy.ndarray:
    """Active sets (iterables of row indices < 64 * words) -> (m, words) uint64 bit masks (include/mpcombi.h,
    mpc_mask_words: 2 words for programs with n_c <= 128, 4 up to 256)."""
    out = numpy.zeros((len(sets), words), dtype=numpy.uint64)
    for i, s in enumerate(sets):
        for v in s:
            out[i, int(v) >> 6] |= numpy.uint64(1) << numpy.uint64(int(v) & 63)
    return out


def masks_to_sets(masks: numpy.ndarray, words: int = MASK_WORDS):
    out = []
    for row in numpy.asarray(masks, dtype=numpy.uint64).reshape(-1, words):
        s = []
        for w in range(words):
            v = int(row[w])
            while v:
                low = v & -v
                s.append(w * 64 + low.bit_length() - 1)
                v ^= low
        out.append(tuple(s))
    return out


def slot_strides(n_x: int, n_t: int, n_c: int, n_tc: int, k: int):
    """(fd, fi): doubles and ints of one slot of a level of cardinality ``k`` (csrc/records.hpp, RecordShape::fd / fi) -- the one copy of
    these formulas on the host side (``Engine.slot_strides``; the multi-GPU driver's engines are not ``Engine`` objects)."""
    return n_x * n_t + n_x + k * n_t + k, 8 + k + n_tc + k + 2 * (n_c - k)


class Engine:
    """One device-resident program (mpc_handle).  Mirrors what every reference worker holds: the presolved
    matrices of the program plus the pruned list; see include/mpcombi.h for the call-by-call mapping."""

    def __init__(self, A, b, F, c, H, Q, A_t, b_t, n_eq: int, device: int = 0, stream: Optional[int] = None):
        L = load()
        self._L = L
        self._h = ctypes.c_void_p()
        self.A, self.b, self.F = _f64(A), _f64(b).reshape(-1), _f64(F)
        self.c, self.H = _f64(c).reshape(-1), _f64(H)
        self.Q = None if Q is None else _f64(Q)
        self.A_t, self.b_t = _f64(A_t), _f64(b_t).reshape(-1)
        self.n_c, self.n_x = self.A.shape
        self.n_t = self.F.shape[1]
        self.n_tc = self.A_t.shape[0]
        self.n_eq = int(n_eq)
        if self.A_t.ndim != 2:
            self.A_t = self.A_t.reshape(self.n_tc, self.n_t)
        p = MpcProblem(self.n_x, self.n_t, self.n_c, self.n_eq, self.n_tc, self.A.ctypes.data_as(_dp),
                       self.b.ctypes.data_as(_dp), self.F.ctypes.data_as(_dp), self.c.ctypes.data_as(_dp),
                       self.H.ctypes.data_as(_dp), None if self.Q is None else self.Q.ctypes.data_as(_dp),
                       self.A_t.ctypes.data_as(_dp) if self.n_tc else None,
                       self.b_t.ctypes.data_as(_dp) if self.n_tc else None)
        rc = L.mpc_create(ctypes.byref(p), int(device), ctypes.c_void_p(stream) if stream else None,
                          ctypes.byref(self._h))
        if rc != MPC_OK:
            raise MpcError(f'mpc_create failed ({rc}): {L.mpc_last_global_error().decode()}')
        self.mask_words = int(L.mpc_mask_words(self._h))
        self.rec_d = int(L.mpc_region_doubles(self._h))
        self.rec_i = int(L.mpc_region_ints(self._h))
        self.device = int(device)
        self._twin = None

    # -- plumbing ----------------------------------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != MPC_OK:
            cls = MpcCapacityError if rc == 3 and what in ('mpc_level_run', 'mpc_level_wait', 'mpc_level_run_batch', 'mpc_solve_wait') else MpcError
            raise cls(f'{what} failed ({rc}): {self._L.mpc_last_error(self._h).decode()}')

    def program_block(self, which: int) -> numpy.ndarray:
        """One of the program's one-off dense blocks as the device holds it (mpc_program_block): 0 W, 1 UV, 2 Gt, 3 X0H, 4 A A';
        5..10: the blocks with the equality rows eliminated (Wr, UVr, (A A')r, Me, Ne, gE; empty when not in use)."""
        n = ctypes.c_int64(0)
        ne = self.n_eq
        shape = {0: (self.n_c, self.n_c), 1: (self.n_c, self.n_t + 1), 2: (self.n_c, self.n_x), 3: (self.n_x, self.n_t + 1),
                 4: (self.n_c, self.n_c), 5: (self.n_c, self.n_c), 6: (self.n_c, self.n_t + 1), 7: (self.n_c, self.n_c),
                 8: (ne, self.n_t + 1), 9: (ne, self.n_c), 10: (2, ne)}[which]
        out = numpy.zeros(shape)
        self._check(self._L.mpc_program_block(self._h, which, out.ctypes.data_as(_dp), out.size, ctypes.byref(n)), 'mpc_program_block')
        return out if n.value else numpy.zeros((0, 0))

    def set_region_overlap(self, on: bool):
        self._check(self._L.mpc_set_region_overlap(self._h, 1 if on else 0), 'mpc_set_region_overlap')

    def set_timing(self, on: bool):
        """HIP-event records around the stages and heavy kernels of this handle's levels (mpc_set_timing): the drivers switch them on
        for the solves that ask for a profile; without them the ms_* fields of the level statistics are 0."""
        on = bool(on)
        if getattr(self, '_timing', None) is not on:
            self._check(self._L.mpc_set_timing(self._h, 1 if on else 0), 'mpc_set_timing')
            self._timing = on

    def engine_kind(self) -> dict:
        """Which kernels this handle's levels run on (mpc_engine_kind)."""
        out = (ctypes.c_int32 * 8)()
        self._check(self._L.mpc_engine_kind(self._h, out), 'mpc_engine_kind')
        return {'register_engine': bool(out[0]), 'rows_per_lane_theta': int(out[1]), 'rows_per_lane_x': int(out[2]), 'rows_per_lane_region': int(out[3]),
                'n_theta_instantiation': int(out[4]), 'theta_open': bool(out[5]), 'kkt_mode': int(out[6]), 'kkt_thread_max_rows': int(out[7])}

    def close(self):
        if getattr(self, '_twin', None) is not None:
            self._twin.close()
            self._twin = None
        if self._h:
            self._L.mpc_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return int(self._L.mpc_stream(self._h) or 0)

    def lds_bytes(self, which: int = 0) -> int:
        return int(self._L.mpc_lds_bytes(self._h, which))

    # -- frontier / pruned list ----------------------------------------------------------------------------------
    def frontier_root(self):
        self._check(self._L.mpc_frontier_root(self._h), 'mpc_frontier_root')

    def frontier_set(self, cands: numpy.ndarray):
        cands = numpy.ascontiguousarray(cands, dtype=numpy.int32)
        n, k = cands.shape
        self._check(self._L.mpc_frontier_set(self._h, cands.ctypes.data_as(_ip), n, k), 'mpc_frontier_set')

    def frontier_set_device(self, ptr: int, n: int, k: int):
        self._check(self._L.mpc_frontier_set_device(self._h, ctypes.c_void_p(ptr), n, k), 'mpc_frontier_set_device')

    def frontier_info(self):
        n, k = ctypes.c_int64(0), ctypes.c_int32(0)
        self._check(self._L.mpc_frontier_info(self._h, ctypes.byref(n), ctypes.byref(k)), 'mpc_frontier_info')
        return n.value, k.value

    def frontier_get(self) -> numpy.ndarray:
        n, k = self.frontier_info()
        out = numpy.zeros((n, k), dtype=numpy.int32)
        if n:
            self._check(self._L.mpc_frontier_get(self._h, out.ctypes.data_as(_ip), n), 'mpc_frontier_get')
        return out

    def pruned_clear(self):
        self._check(self._L.mpc_pruned_clear(self._h), 'mpc_pruned_clear')

    def pruned_add(self, masks: numpy.ndarray):
        masks = numpy.ascontiguousarray(masks, dtype=numpy.uint64).reshape(-1, self.mask_words)
        if len(masks):
            self._check(self._L.mpc_pruned_add(self._h, masks.ctypes.data_as(_u64p), len(masks)), 'mpc_pruned_add')

    def pruned_add_device(self, ptr: int, m: int):
        self._check(self._L.mpc_pruned_add_device(self._h, ctypes.c_void_p(ptr), m), 'mpc_pruned_add_device')

    def frontier_shard(self, rank: int, world: int):
        self._check(self._L.mpc_frontier_shard(self._h, rank, world), 'mpc_frontier_shard')

    def pruned_count(self) -> int:
        return int(self._L.mpc_pruned_count(self._h))

    def pruned_get(self) -> numpy.ndarray:
        m = self.pruned_count()
        out = numpy.zeros((m, self.mask_words), dtype=numpy.uint64)
        if m:
            self._check(self._L.mpc_pruned_get(self._h, out.ctypes.data_as(_u64p), m), 'mpc_pruned_get')
        return out

    # -- one level --------------------------------------------------------------------------------------------------
    def level_run(self, gen_children: bool, graph: bool = False, keep_lowdim: bool = False, stream: bool = False) -> LevelStats:
        """One level over the resident frontier.  ``graph``: the question of the connected-graph traversal (MPC_LEVEL_GRAPH);
        ``keep_lowdim``: the serial driver's expansion rule (MPC_LEVEL_KEEP_LOWDIM); ``stream``: the region records are
        written into page-locked host arrays, complete on return, handed over by ``level_stream_info()``."""
        st = LevelStats()
        self._check(self._L.mpc_level_run_ex(self._h, int(bool(gen_children)), (MPC_LEVEL_GRAPH if graph else 0)
                                             | (MPC_LEVEL_KEEP_LOWDIM if keep_lowdim else 0) | (MPC_LEVEL_STREAM if stream else 0),
                                             ctypes.byref(st)), 'mpc_level_run')
        self._last = st
        return st

    @staticmethod
    def frontier_advance_batch(engines):
        """``frontier_advance`` for many engines with one call into the library (mpc_frontier_advance_batch)."""
        B = len(engines)
        if B:
            hs = (ctypes.c_void_p * B)(*[e._h for e in engines])
            rc = engines[0]._L.mpc_frontier_advance_batch(hs, B)
            if rc != 0:
                Engine._raise_for(engines, rc)

    def level_memory_gb(self, gen_children: bool) -> float:
        """Device memory (GB) the next level of this engine's frontier holds in a batch (mpc_level_memory_gb)."""
        return float(self._L.mpc_level_memory_gb(self._h, int(bool(gen_children))))

    def trim(self):
        """Gives the level buffers back to the pool (mpc_trim); the program stays usable."""
        self._check(self._L.mpc_trim(self._h), 'mpc_trim')

    @staticmethod
    def level_batch_start(engines, gen_children, keep_lowdim: bool = False):
        """First half of ``level_run_batch`` (mpc_level_batch_start): queues the shared launches of one level for all engines and
        returns a token for ``level_batch_wait``; the engines must not be touched in between."""
        B = len(engines)
        L = engines[0]._L
        hs = (ctypes.c_void_p * B)(*[e._h for e in engines])
        gc = (ctypes.c_int32 * B)(*[int(bool(g)) for g in gen_children])
        tok = ctypes.c_void_p()
        rc = L.mpc_level_batch_start(hs, B, gc, MPC_LEVEL_KEEP_LOWDIM if keep_lowdim else 0, ctypes.byref(tok))
        if rc != 0:
            Engine._raise_for(engines, rc)
        return (tok, list(engines))

    @staticmethod
    def level_batch_wait(token):
        """Second half: ([LevelStats per engine], members that went through the shared launches)."""
        tok, engines = token
        B = len(engines)
        stats = (LevelStats * B)()
        nb = ctypes.c_int32(0)
        rc = engines[0]._L.mpc_level_batch_wait(tok, stats, ctypes.byref(nb))
        if rc != 0:
            Engine._raise_for(engines, rc)
        out = list(stats)               # elements are views that keep the array alive
        for e, st in zip(engines, out):
            e._last = st
        return out, int(nb.value)

    def slot_strides(self, k: int):
        return slot_strides(self.n_x, self.n_t, self.n_c, self.n_tc, k)

    def _rows_cap(self, st) -> int:
        """Upper bound of the rows the level's records own, from its LevelStats (csrc/records.hpp, record_rows_bound): pooled rows + a
        full row block per candidate the LDS-engine kernel re-solved; a level built by that kernel alone (no register-resident
        instantiation: one parameter) reports no pooled rows."""
        nr, rows_t = int(st.n_regions), self.n_c - self.n_eq + self.n_tc
        if not nr:
            return 0
        return int(st.n_region_rows) + int(st.n_region_retry) * rows_t if st.n_region_rows else nr * rows_t

    @staticmethod
    def level_batch_fetch(engines):
        """``level_regions_slots_nowait`` for many engines with ONE call into the library and THREE page-locked blocks for all of
        them (the members' arrays are views into those): [(head_d, head_i, erows, k) per engine], copies queued only.  Sizes come from
        each engine's LevelStats of the level just run."""
        B = len(engines)
        if B == 0:
            return []
        fds, fis, nss, nrs = [], [], [], []
        for e in engines:
            st = e._last
            fd, fi = e.slot_strides(int(st.k))
            fds.append(fd)
            fis.append(fi)
            nss.append(int(st.n_opt) if st.n_regions else 0)
            nrs.append(e._rows_cap(st))
        od = numpy.concatenate([[0], numpy.cumsum([n * f for n, f in zip(nss, fds)])]).astype(numpy.int64)
        oi = numpy.concatenate([[0], numpy.cumsum([n * f for n, f in zip(nss, fis)])]).astype(numpy.int64)
        oe = numpy.concatenate([[0], numpy.cumsum([n * (e.n_t + 1) for n, e in zip(nrs, engines)])]).astype(numpy.int64)
        big_d = pinned_empty((max(int(od[-1]), 1),), numpy.float64)
        big_i = pinned_empty((max(int(oi[-1]), 1),), numpy.int32)
        big_e = pinned_empty((max(int(oe[-1]), 1),), numpy.float64)
        pd = (ctypes.c_void_p * B)(*(big_d.ctypes.data + 8 * od[:-1]).tolist())
        pi = (ctypes.c_void_p * B)(*(big_i.ctypes.data + 4 * oi[:-1]).tolist())
        pe = (ctypes.c_void_p * B)(*(big_e.ctypes.data + 8 * oe[:-1]).tolist())
        caps = (ctypes.c_int64 * B)(*nss)
        capr = (ctypes.c_int64 * B)(*nrs)
        n1 = (ctypes.c_int64 * B)()
        n2 = (ctypes.c_int64 * B)()
        hs = (ctypes.c_void_p * B)(*[e._h for e in engines])
        rc = engines[0]._L.mpc_level_batch_fetch(hs, B, pd, pi, caps, pe, capr, n1, n2)
        if rc != 0:
            Engine._raise_for(engines, rc)
        # (the members' arrays are complete after Engine.fetch_wait / any member's sync / the next level_batch_start)
        out = []
        for j, e in enumerate(engines):
            ns, nr = int(n1[j]), int(n2[j])
            out.append((big_d[od[j]:od[j] + ns * fds[j]].reshape(ns, fds[j]), big_i[oi[j]:oi[j] + ns * fis[j]].reshape(ns, fis[j]),
                        big_e[oe[j]:oe[j] + nr * (e.n_t + 1)].reshape(nr, e.n_t + 1), int(e._last.k)))
        return out

    @staticmethod
    def solve_many_start(engines, max_levels, keep_lowdim: bool = False, base: bool = False):
        """The level loop of all ``engines`` on a thread of the library (mpc_solve_many_start): every engine's pruned list is cleared, its
        frontier rooted, then level after level with shared launches; returns the job for ``solve_many_level`` / ``solve_many_wait``.
        The engines must not be touched until ``solve_many_wait`` has returned."""
        B = len(engines)
        hs = (ctypes.c_void_p * B)(*[e._h for e in engines])
        ml = (ctypes.c_int32 * B)(*[int(v) for v in max_levels])
        job = ctypes.c_void_p()
        rc = engines[0]._L.mpc_solve_many_start(hs, B, ml, (MPC_LEVEL_KEEP_LOWDIM if keep_lowdim else 0) | (MPC_SOLVE_MANY_BASE if base else 0), ctypes.byref(job))
        if rc != 0:
            Engine._raise_for(engines, rc)
        return (job, list(engines))

    @staticmethod
    def solve_many_level(job, level: int):
        """Blocks until level ``level`` of the job has been run and its records are complete (mpc_solve_many_level).  Returns
        ``(done, None)`` past the last level (done = 1: all members finished, 2: the caller takes over -- memory budget), else
        ``(0, (members, stats, n_shared, ms_wall, records, base))`` (``base``: the closing level of the base active sets) with ``records`` = [(member, head_d, head_i, erows, k)] for the members
        that found regions (views into three page-locked blocks that return to the pool with their last view)."""
        jb, engines = job
        info = ManyLevelInfo()
        rc = engines[0]._L.mpc_solve_many_level(jb, int(level), ctypes.byref(info))
        if rc != 0:
            Engine._raise_for(engines, rc)
        nm = int(info.n_members)
        if nm == 0:
            return int(info.done), None
        members = info.member[:nm]
        # copies: info.stats[j] is a view into the job's own vector, which mpc_solve_many_wait frees (the engines keep `_last`)
        stats = [LevelStats.from_buffer_copy(info.stats[j]) for j in range(nm)]
        for i, st in zip(members, stats):
            engines[i]._last = st
        records = []
        if info.head_d:
            big_d = pinned_adopt(info.head_d, (int(info.len_d),), numpy.float64)
            big_i = pinned_adopt(info.head_i, (int(info.len_i),), numpy.int32)
            big_e = pinned_adopt(info.erows, (max(int(info.len_e), 1),), numpy.float64)
            ns, nr, od, oi, oe = info.n_slots[:nm], info.n_rows[:nm], info.off_d[:nm], info.off_i[:nm], info.off_e[:nm]
            for j, i in enumerate(members):
                if ns[j] == 0:
                    continue
                e, k = engines[i], int(stats[j].k)
                fd, fi = e.slot_strides(k)
                records.append((i, big_d[od[j]:od[j] + ns[j] * fd].reshape(ns[j], fd), big_i[oi[j]:oi[j] + ns[j] * fi].reshape(ns[j], fi),
                                big_e[oe[j]:oe[j] + nr[j] * (e.n_t + 1)].reshape(nr[j], e.n_t + 1), k))
        return 0, (members, stats, int(info.n_shared), float(info.ms_wall), records, bool(info.base))

    @staticmethod
    def solve_many_wait(job):
        """Joins the loop and frees the job (mpc_solve_many_wait); raises what the loop failed with."""
        jb, engines = job
        rc = engines[0]._L.mpc_solve_many_wait(jb)
        if rc != 0:
            Engine._raise_for(engines, rc)

    @staticmethod
    def fetch_wait(engine):
        """Waits for the shared record copy of the last ``level_batch_fetch`` on the engine's device (mpc_fetch_wait)."""
        rc = engine._L.mpc_fetch_wait(int(engine.device))
        if rc != 0:
            engine._check(rc, 'mpc_fetch_wait')

    @staticmethod
    def _raise_for(engines, rc):
        for e in engines:      # the failing member carries the message
            if e._L.mpc_last_error(e._h):
                e._check(rc, 'mpc_level_run_batch')
        engines[0]._check(rc, 'mpc_level_run_batch')

    @staticmethod
    def level_run_batch(engines, gen_children, keep_lowdim: bool = False):
        """One level of several programs per launch (mpc_level_run_batch): ``engines`` are distinct Engines on one device, each
        with its frontier; ``gen_children`` one flag per engine.  Returns ([LevelStats per engine], members that went through the
        shared launches).  Afterwards every engine is in the state ``level_run`` would have left it in."""
        return Engine.level_batch_wait(Engine.level_batch_start(engines, gen_children, keep_lowdim))

    # -- the same level on the handle's worker thread, region records streamed to the host (include/mpcombi.h) ----------
    def level_start(self, gen_children: bool, stream: bool = True, then_base: bool = False, keep_lowdim: bool = False,
                    only_base: bool = False):
        self._check(self._L.mpc_level_start(self._h, int(bool(gen_children)),
                                            (MPC_LEVEL_STREAM if stream else 0) | (MPC_LEVEL_THEN_BASE if then_base else 0)
                                            | (MPC_LEVEL_KEEP_LOWDIM if keep_lowdim else 0)
                                            | (MPC_LEVEL_ONLY_BASE if only_base else 0)), 'mpc_level_start')

    def twin(self) -> 'Engine':
        """A second handle of the same program on the same device (created on first use, ~0.5 ms): the solve loop runs the
        base-set check there (``level_start(False, only_base=True)``) while this handle works on its large levels."""
        if self._twin is None:
            self._twin = Engine(self.A, self.b, self.F, self.c, self.H, self.Q, self.A_t, self.b_t, self.n_eq, device=self.device)
        return self._twin

    def base_result(self):
        """(status, rec_d [1, rec_d] or empty, rec_i) of the base-set check the worker ran behind the last level
        (``level_start(..., then_base=True)``), or None when it did not run."""
        status = numpy.zeros(1, dtype=numpy.uint8)
        nreg = ctypes.c_int64(0)
        d = numpy.zeros((1, self.rec_d))
        i = numpy.zeros((1, self.rec_i), dtype=numpy.int32)
        rc = self._L.mpc_base_result(self._h, status.ctypes.data_as(_u8p), ctypes.byref(nreg), d.ctypes.data_as(_dp), i.ctypes.data_as(_ip))
        if rc != MPC_OK:
            return None
        return status, d[:nreg.value], i[:nreg.value]

    def level_stream_info(self):
        """Blocks until the running level's region stage has been launched.  None when the level does not stream, else
        (head_d [S, fd], head_i [S, fi], erows [cap_rows, n_t+1], chunk, n_chunks) -- arrays the region kernel is writing;
        chunk j (slots j*chunk ...) may be read after ``level_chunk_wait(j)``."""
        hd, hi, er = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        ns, cr, ch, nch = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._L.mpc_level_stream_info(self._h, ctypes.byref(hd), ctypes.byref(hi), ctypes.byref(er), ctypes.byref(ns),
                                                  ctypes.byref(cr), ctypes.byref(ch), ctypes.byref(nch)), 'mpc_level_stream_info')
        if ns.value == 0:
            return None
        n, k = self.frontier_info()
        fd, fi = self.slot_strides(k)
        return (pinned_adopt(hd.value, (ns.value, fd), numpy.float64), pinned_adopt(hi.value, (ns.value, fi), numpy.int32),
                pinned_adopt(er.value, (max(cr.value, 1), self.n_t + 1), numpy.float64), int(ch.value), int(nch.value))

    def level_chunk_wait(self, j: int):
        self._check(self._L.mpc_level_chunk_wait(self._h, int(j)), 'mpc_level_chunk_wait')

    def level_wait(self) -> LevelStats:
        st = LevelStats()
        self._check(self._L.mpc_level_wait(self._h, ctypes.byref(st)), 'mpc_level_wait')
        self._last = st
        return st

    def level_stream_fixup(self, hd, hi, er) -> int:
        """Fills the slots of candidates the LDS-engine kernel re-solved (stats.n_region_retry > 0); returns the rows in use."""
        nrows = ctypes.c_int64(0)
        self._check(self._L.mpc_level_stream_fixup(self._h, hd.ctypes.data_as(_dp), hi.ctypes.data_as(_ip), er.ctypes.data_as(_dp),
                                                   ctypes.byref(nrows)), 'mpc_level_stream_fixup')
        return int(nrows.value)

    # -- the whole level loop on the handle's worker thread (include/mpcombi.h, mpc_solve_*) ---------------------------------
    def solve_start(self, max_levels: int, stream: bool = True, fetch: bool = True, then_base: bool = False, keep_lowdim: bool = False):
        self._check(self._L.mpc_solve_start(self._h, int(max_levels), (MPC_LEVEL_STREAM if stream else 0) | (MPC_SOLVE_FETCH if fetch else 0)
                                            | (MPC_LEVEL_THEN_BASE if then_base else 0) | (MPC_LEVEL_KEEP_LOWDIM if keep_lowdim else 0)), 'mpc_solve_start')

    def solve_level(self, level: int):
        """Blocks until level ``level`` of the running solve has records to hand over or has finished.  None: the loop ended before
        this level.  Else (mode, k, n, head_d, head_i, erows, chunk, n_chunks): mode 1 = arrays the region kernel is still writing
        (chunk j readable after ``solve_chunk_wait(level, j)``), 2 = complete arrays, 0 = no records (arrays None)."""
        info = SolveLevelInfo()
        rc = self._L.mpc_solve_level(self._h, int(level), ctypes.byref(info))
        if info.mode < 0:
            return None
        self._check(rc, 'mpc_solve_level')
        if info.mode == 0:
            return 0, int(info.k), int(info.n), None, None, None, 0, 0
        k = int(info.k)
        fd, fi = self.slot_strides(k)
        ns = int(info.n_slots)
        return (int(info.mode), k, int(info.n), pinned_adopt(info.head_d, (ns, fd), numpy.float64), pinned_adopt(info.head_i, (ns, fi), numpy.int32),
                pinned_adopt(info.erows, (max(int(info.n_rows), 1), self.n_t + 1), numpy.float64), int(info.chunk), int(info.n_chunks))

    def solve_chunk_wait(self, level: int, j: int):
        self._check(self._L.mpc_solve_chunk_wait(self._h, int(level), int(j)), 'mpc_solve_chunk_wait')

    def solve_level_wait(self, level: int):
        """(LevelStats, wall milliseconds) of a finished level of the running solve."""
        st = LevelStats()
        ms = ctypes.c_double(0.0)
        self._check(self._L.mpc_solve_level_wait(self._h, int(level), ctypes.byref(st), ctypes.byref(ms)), 'mpc_solve_level_wait')
        self._last = st
        return st, float(ms.value)

    def solve_wait(self) -> int:
        """Joins the solve loop; raises what the loop failed with (MpcCapacityError as for ``level_wait``); levels completed."""
        nl = ctypes.c_int32(0)
        self._check(self._L.mpc_solve_wait(self._h, ctypes.byref(nl)), 'mpc_solve_wait')
        return int(nl.value)

    def qp_solve_batch(self, thetas: numpy.ndarray):
        """The program's QP at every row of ``thetas`` [m, n_t] (positive definite Q), one wavefront per point:
        (status [m] (0 optimal, 1 infeasible, 3 iteration limit), x [m, n_x], lambda [m, n_c], active [m, n_c] bool)."""
        th = _f64(thetas).reshape(-1, self.n_t)
        m = len(th)
        status = numpy.zeros(m, dtype=numpy.int32)
        x = numpy.zeros((m, self.n_x))
        lam = numpy.zeros((m, self.n_c))
        act = numpy.zeros((m, self.n_c), dtype=numpy.uint8)
        self._check(self._L.mpc_qp_solve_batch(self._h, m, th.ctypes.data_as(_dp), status.ctypes.data_as(_ip), x.ctypes.data_as(_dp),
                                               lam.ctypes.data_as(_dp), act.ctypes.data_as(_u8p), None), 'mpc_qp_solve_batch')
        return status, x, lam, act.astype(bool)

    # -- connected-graph traversal with the bookkeeping on the device (include/mpcombi.h, mpc_graph_*) -------------------
    def graph_begin(self, seed_masks: numpy.ndarray, variant: int):
        m = numpy.ascontiguousarray(seed_masks, dtype=numpy.uint64).reshape(-1, self.mask_words)
        self._check(self._L.mpc_graph_begin(self._h, m.ctypes.data_as(_u64p), len(m), int(variant)), 'mpc_graph_begin')

    def graph_wave(self):
        """[(cardinality, number of active sets)] of the current wave (empty: the traversal is complete), sets queued so far."""
        cap = 600
        ks = numpy.zeros(cap, dtype=numpy.int32)
        cs = numpy.zeros(cap, dtype=numpy.int64)
        ng = ctypes.c_int32(0)
        nw, nv = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._L.mpc_graph_wave(self._h, ks.ctypes.data_as(_ip), cs.ctypes.data_as(_lp), cap, ctypes.byref(ng), ctypes.byref(nw),
                                           ctypes.byref(nv)), 'mpc_graph_wave')
        return list(zip(ks[:ng.value].tolist(), cs[:ng.value].tolist())), int(nv.value)

    def graph_group_run(self, group: int) -> LevelStats:
        st = LevelStats()
        self._check(self._L.mpc_graph_group_run(self._h, int(group), ctypes.byref(st)), 'mpc_graph_group_run')
        self._last = st
        return st

    def graph_wave_close(self):
        nn, nv = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._L.mpc_graph_wave_close(self._h, ctypes.byref(nn), ctypes.byref(nv)), 'mpc_graph_wave_close')
        return int(nn.value), int(nv.value)

    def level_status(self) -> numpy.ndarray:
        n, _ = self.frontier_info()
        out = numpy.zeros(n, dtype=numpy.uint8)
        if n:
            self._check(self._L.mpc_level_status(self._h, out.ctypes.data_as(_u8p)), 'mpc_level_status')
        return out

    def level_regions(self):
        nr = int(self._last.n_regions)
        d = numpy.zeros((nr, self.rec_d))
        i = numpy.zeros((nr, self.rec_i), dtype=numpy.int32)
        idx = numpy.zeros(nr, dtype=numpy.int64)
        if nr:
            self._check(self._L.mpc_level_regions(self._h, d.ctypes.data_as(_dp), i.ctypes.data_as(_ip),
                                                  idx.ctypes.data_as(_lp), nr), 'mpc_level_regions')
        return d, i, idx

    def level_regions_compact(self):
        """Regions of the level in the device's compact form: (head_d [n, fd], head_i [n, fi], erows [R, n_t+1], k)."""
        nr = int(self._last.n_regions)
        fd, fi, mr = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._L.mpc_compact_strides(self._h, ctypes.byref(fd), ctypes.byref(fi), ctypes.byref(mr)),
                    'mpc_compact_strides')
        k = int(self._last.k)
        rows_cap = int(mr.value) if nr else 0
        hd = numpy.empty((nr, fd.value))
        hi = numpy.empty((nr, fi.value), dtype=numpy.int32)
        er = numpy.empty((max(rows_cap, 1), self.n_t + 1))
        n1, n2 = ctypes.c_int64(0), ctypes.c_int64(0)
        if nr:
            self._check(self._L.mpc_level_regions_compact(self._h, hd.ctypes.data_as(_dp), hi.ctypes.data_as(_ip), nr,
                                                          er.ctypes.data_as(_dp), rows_cap, ctypes.byref(n1),
                                                          ctypes.byref(n2)), 'mpc_level_regions_compact')
        return hd[:n1.value], hi[:n1.value], er[:n2.value], k

    def sync(self):
        """Waits for everything queued on the handle's stream (completes an asynchronous slot fetch)."""
        self._check(self._L.mpc_sync(self._h), 'mpc_sync')

    def level_regions_slots_nowait(self):
        """``level_regions_slots`` that only QUEUES the copies: (head_d, head_i, erows, k) -- all three complete after ``sync()`` or
        the next level of this engine; then ``numpy.flatnonzero(head_i[:, 0] == REGION)`` are the region slots."""
        nr = int(self._last.n_regions)
        fd, fi, mr = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._L.mpc_compact_strides(self._h, ctypes.byref(fd), ctypes.byref(fi), ctypes.byref(mr)), 'mpc_compact_strides')
        ns = int(self._L.mpc_level_slots(self._h)) if nr else 0
        rows_cap = int(mr.value) if nr else 0
        hd = pinned_empty((ns, fd.value), numpy.float64)
        hi = pinned_empty((ns, fi.value), numpy.int32)
        er = pinned_empty((max(rows_cap, 1), self.n_t + 1), numpy.float64)
        n1, n2 = ctypes.c_int64(0), ctypes.c_int64(0)
        if nr:
            self._check(self._L.mpc_level_regions_slots_nowait(self._h, hd.ctypes.data_as(_dp), hi.ctypes.data_as(_ip), ns, er.ctypes.data_as(_dp),
                                                               rows_cap, ctypes.byref(n1), ctypes.byref(n2)), 'mpc_level_regions_slots')
        return hd[:n1.value], hi[:n1.value], er[:n2.value], int(self._last.k)

    def level_regions_slots(self, early_return: bool = False):
        """All slots the region kernel wrote for this level, copied by DMA into pooled page-locked arrays:
        (head_d [S, fd], head_i [S, fi], erows [R, n_t+1], k, region_slots) -- region_slots = the slots that are regions.
        ``early_return``: come back when head_i is there; head_d and erows are complete after ``sync()`` (or the next
        ``level_run``) -- the caller must not read them before."""
        nr = int(self._last.n_regions)
        fd, fi, mr = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._L.mpc_compact_strides(self._h, ctypes.byref(fd), ctypes.byref(fi), ctypes.byref(mr)),
                    'mpc_compact_strides')
        k = int(self._last.k)
        ns = int(self._L.mpc_level_slots(self._h)) if nr else 0
        rows_cap = int(mr.value) if nr else 0
        hd = pinned_empty((ns, fd.value), numpy.float64)
        hi = pinned_empty((ns, fi.value), numpy.int32)
        er = pinned_empty((max(rows_cap, 1), self.n_t + 1), numpy.float64)
        n1, n2 = ctypes.c_int64(0), ctypes.c_int64(0)
        if nr:
            fetch = self._L.mpc_level_regions_slots_async if early_return else self._L.mpc_level_regions_slots
            self._check(fetch(self._h, hd.ctypes.data_as(_dp), hi.ctypes.data_as(_ip), ns, er.ctypes.data_as(_dp), rows_cap,
                              ctypes.byref(n1), ctypes.byref(n2)), 'mpc_level_regions_slots')
        hi = hi[:n1.value]
        return hd[:n1.value], hi, er[:n2.value], k, numpy.flatnonzero(hi[:, 0] == REGION)

    def level_children(self) -> numpy.ndarray:
        n = int(self._last.n_children)
        out = numpy.zeros((n, int(self._last.k) + 1), dtype=numpy.int32)
        if n:
            self._check(self._L.mpc_level_children(self._h, out.ctypes.data_as(_ip), n), 'mpc_level_children')
        return out

    def level_children_device(self, ptr: int, cap: int):
        self._check(self._L.mpc_level_children_device(self._h, ctypes.c_void_p(ptr), cap), 'mpc_level_children_device')

    def level_pruned_new(self) -> numpy.ndarray:
        m = int(self._last.n_pruned_new)
        out = numpy.zeros((m, self.mask_words), dtype=numpy.uint64)
        if m:
            self._check(self._L.mpc_level_pruned_new(self._h, out.ctypes.data_as(_u64p), m), 'mpc_level_pruned_new')
        return out

    def level_region_shapes(self):
        """(slots, fd, fi, row capacity) of the level just run: the shapes level_regions_device fills."""
        fd, fi, mr = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._L.mpc_compact_strides(self._h, ctypes.byref(fd), ctypes.byref(fi), ctypes.byref(mr)),
                    'mpc_compact_strides')
        ns = int(self._L.mpc_level_slots(self._h)) if int(self._last.n_regions) else 0
        return ns, int(fd.value), int(fi.value), int(mr.value) if ns else 0

    def level_regions_device(self, hd_ptr: int, hi_ptr: int, er_ptr: int, cap_slots: int, cap_rows: int):
        """Slot arrays device -> device into caller-owned device buffers; (n_slots, n_rows), or None when some record
        of the level only exists in the host route's form (then use level_regions_slots)."""
        n1, n2 = ctypes.c_int64(0), ctypes.c_int64(0)
        rc = self._L.mpc_level_regions_device(self._h, ctypes.c_void_p(hd_ptr), ctypes.c_void_p(hi_ptr),
                                              ctypes.c_void_p(er_ptr), cap_slots, cap_rows, ctypes.byref(n1), ctypes.byref(n2))
        if rc == 4:      # MPC_ERR_STATE
            return None
        self._check(rc, 'mpc_level_regions_device')
        return int(n1.value), int(n2.value)

    def level_pruned_new_device(self, ptr: int, cap: int):
        self._check(self._L.mpc_level_pruned_new_device(self._h, ctypes.c_void_p(ptr), cap),
                    'mpc_level_pruned_new_device')

    def frontier_advance(self):
        self._check(self._L.mpc_frontier_advance(self._h), 'mpc_frontier_advance')

    # -- the host-buffer operator (pool.map(full_process) replacement) --------------------------------------------
    def check_level(self, cands: numpy.ndarray, pruned_masks: numpy.ndarray, gen_children: bool):
        cands = numpy.ascontiguousarray(cands, dtype=numpy.int32)
        n, k = cands.shape
        pm = numpy.ascontiguousarray(pruned_masks, dtype=numpy.uint64).reshape(-1, self.mask_words)
        status = numpy.zeros(n, dtype=numpy.uint8)
        nreg, nch = ctypes.c_int64(0), ctypes.c_int64(0)
        # small levels: capacities that cannot be exceeded, so one call suffices; large levels: ask first
        rcap = n if n <= 4096 else 0
        ccap = n * self.n_c if (gen_children and n <= 4096) else 0
        for _ in range(2):
            d = numpy.zeros((max(rcap, 1), self.rec_d))
            i = numpy.zeros((max(rcap, 1), self.rec_i), dtype=numpy.int32)
            idx = numpy.zeros(max(rcap, 1), dtype=numpy.int64)
            ch = numpy.zeros((max(ccap, 1), k + 1), dtype=numpy.int32)
            rc = self._L.mpc_check_level(self._h, cands.ctypes.data_as(_ip), n, k, pm.ctypes.data_as(_u64p), len(pm),
                                         int(bool(gen_children)), status.ctypes.data_as(_u8p), ctypes.byref(nreg),
                                         d.ctypes.data_as(_dp), i.ctypes.data_as(_ip), idx.ctypes.data_as(_lp), rcap,
                                         ctypes.byref(nch), ch.ctypes.data_as(_ip), ccap)
            if rc == MPC_ERR_CAPACITY:
                rcap, ccap = nreg.value, nch.value
                continue
            self._check(rc, 'mpc_check_level')
            break
        return status, d[:nreg.value], i[:nreg.value], idx[:nreg.value], ch[:nch.value]


def lp_solve_batch(A, b, c, eq_flags, device: int = 0, want_x: bool = True):
    """Batched LPs on the device.  A: (n_lp, m, n) or (m, n) shared; b likewise; c (n_lp, n) / (n,) / None;
    eq_flags: (n_lp, m) bool.  Returns (status, x, obj, iterations); x is None with ``want_x=False`` (nothing is
    allocated or copied back for it)."""
    L = load()
    A = _f64(A)
    eq_flags = numpy.ascontiguousarray(eq_flags, dtype=numpy.uint8)
    n_lp, m = eq_flags.shape
    shared_A = A.ndim == 2
    n = A.shape[-1]
    b = _f64(b)
    shared_b = b.size == m and n_lp != 1 or b.size == m
    if b.size != m:
        shared_b = False
    cp, shared_c = None, 1
    if c is not None:
        c = _f64(c)
        shared_c = int(c.size == n)
        cp = c.ctypes.data_as(_dp)
    status = numpy.zeros(n_lp, dtype=numpy.int32)
    x = numpy.zeros((n_lp, n)) if want_x else None
    obj = numpy.zeros(n_lp)
    it = numpy.zeros(n_lp, dtype=numpy.int32)
    rc = L.mpc_lp_solve_batch(int(device), n_lp, m, n, A.ctypes.data_as(_dp), int(shared_A), b.ctypes.data_as(_dp),
                              int(shared_b), cp, shared_c, eq_flags.ctypes.data_as(_u8p), status.ctypes.data_as(_ip),
                              None if x is None else x.ctypes.data_as(_dp), obj.ctypes.data_as(_dp), it.ctypes.data_as(_ip))
    if rc != MPC_OK:
        raise MpcError(f'mpc_lp_solve_batch failed ({rc}): {L.mpc_last_global_error().decode()}')
    return status, x, obj, it


def miqp_solve_batch(blocks: dict, Y: numpy.ndarray, theta: numpy.ndarray, device: int = 0, want_x: bool = True):
    """The mixed-integer QP at every row of theta (include/mpcombi.h, mpc_miqp_solve_batch): the LCP of every (point, leaf) pair,
    the best leaf per point (lowest objective, lowest leaf on ties), the winners' outputs.  ``blocks``: the arrays of
    MPMIQP_Program.theta_blocks; Y [n_leaves, n_b] the fixations.  Device memory is 12 bytes per (point, leaf): the caller bounds
    len(theta).  Returns (status [m], leaf [m], obj [m], x [m, n_x] or None, lambda [m, n_rows] or None, active [m, n_rows] or None)."""
    L = load()
    B = blocks
    n_c, n_eq, n_x, n_t, n_b, n_rows = (int(B[k]) for k in ('n_c', 'n_eq', 'n_x', 'n_t', 'n_b', 'n_rows'))
    arr = {k: _f64(B[k]) for k in ('W', 'UV', 'X0', 'Gt', 'Q_c', 'G', 'K', 'check')}
    check_eq = numpy.ascontiguousarray(B['check_eq'], dtype=numpy.uint8)
    bins = numpy.ascontiguousarray(B['binary_index'], dtype=numpy.int32)
    lcp_row = numpy.ascontiguousarray(B['lcp_row'], dtype=numpy.int32)
    Y = _f64(numpy.asarray(Y, dtype=numpy.float64).reshape(-1, n_b))
    th = _f64(numpy.asarray(theta, dtype=numpy.float64).reshape(-1, n_t))
    m, n_leaves = len(th), len(Y)
    status, leaf, obj = numpy.zeros(m, dtype=numpy.int32), numpy.zeros(m, dtype=numpy.int32), numpy.zeros(m)
    x = numpy.zeros((m, n_x)) if want_x else None
    lam = numpy.zeros((m, n_rows)) if want_x else None
    act = numpy.zeros((m, n_rows), dtype=numpy.uint8) if want_x else None
    p = lambda a, t=_dp: None if a is None else a.ctypes.data_as(t)
    rc = L.mpc_miqp_solve_batch(int(device), n_c, n_eq, n_x, n_t, n_b, *(p(arr[k]) for k in ('W', 'UV', 'X0', 'Gt', 'Q_c', 'G', 'K')),
                                int(arr['check'].shape[0]), p(arr['check']), p(check_eq, _u8p), p(bins, _ip), n_rows, p(lcp_row, _ip),
                                n_leaves, p(Y), m, p(th), p(status, _ip), p(leaf, _ip), p(obj), p(x), p(lam), p(act, _u8p))
    if rc != MPC_OK:
        raise MpcError(f'mpc_miqp_solve_batch failed ({rc}): {L.mpc_last_global_error().decode()}')
    return status, leaf, obj, x, lam, act


def hit_and_run(row_off, ab_rows, start, chains: int, samples: int, n_steps: int, seed: int, device: int = 0):
    """Hit-and-run chains in a batch of polytopes {x : A_p x <= b_p} (include/mpcombi.h, mpc_hit_and_run; the chain is specified in
    DESIGN §3.11).  ab_rows [total_rows, n+1] = [b | A] stacked, row_off [n_poly+1], start [n_poly, n].  Returns
    (samples [n_poly, chains, samples, n], status [n_poly, chains]) with status MPC_HR_*; a chain whose status is not MPC_HR_OK
    has NaN samples.  The time of the kernel is left in ``hit_and_run.last_ms``.  Bad sizes raise MpcError before any launch."""
    off = numpy.ascontiguousarray(row_off, dtype=numpy.int64).reshape(-1)
    ab = _f64(numpy.asarray(ab_rows, dtype=numpy.float64))
    n_poly = len(off) - 1
    st = _f64(numpy.asarray(start, dtype=numpy.float64))
    chains, samples, n_steps, seed = int(chains), int(samples), int(n_steps), int(seed)
    if n_poly < 0 or ab.ndim != 2 or st.ndim != 2 or st.shape[0] != n_poly:
        raise MpcError('hit_and_run: row_off [n_poly+1], ab_rows [rows, n+1] and start [n_poly, n] do not fit together')
    n = st.shape[1]
    if ab.shape[1] != n + 1 or ab.shape[0] != (int(off[-1]) if n_poly >= 0 else 0):
        raise MpcError(f'hit_and_run: ab_rows has shape {ab.shape}, expected ({int(off[-1])}, {n + 1})')
    if not 1 <= n <= HR_MAX_DIM:
        raise MpcError(f'hit_and_run: dimension {n} outside 1..{HR_MAX_DIM}')
    if off[0] != 0 or numpy.any(numpy.diff(off) < 0) or numpy.any(numpy.diff(off) > HR_MAX_ROWS):
        raise MpcError(f'hit_and_run: row_off must start at 0 and give 0..{HR_MAX_ROWS} rows per polytope')
    if chains < 0 or samples < 1 or n_steps < 1 or samples * n_steps >= 1 << 32 or not 0 <= seed < 1 << 64:
        raise MpcError('hit_and_run: need chains >= 0, samples >= 1, n_steps >= 1, samples * n_steps < 2^32 and a 64-bit seed')
    L = load()
    out = numpy.empty((n_poly, chains, samples, n))
    status = numpy.zeros((n_poly, chains), dtype=numpy.int32)
    ms = ctypes.c_float(0.0)
    rc = L.mpc_hit_and_run(int(device), n, n_poly, off.ctypes.data_as(_lp), ab.ctypes.data_as(_dp), st.ctypes.data_as(_dp), chains, samples,
                           n_steps, seed, out.ctypes.data_as(_dp), status.ctypes.data_as(_ip), ctypes.byref(ms))
    if rc != MPC_OK:
        raise MpcError(f'mpc_hit_and_run failed ({rc}): {L.mpc_last_global_error().decode()}')
    hit_and_run.last_ms = float(ms.value)
    return out, status


hit_and_run.last_ms = 0.0


def region_vertices(row_off, ef_rows, n_t: int, tol: float = 1e-9, slab: int = 0, max_slab: int = 0, budget: int = 0, device: int = 0):
    """mpc_region_vertices: the vertices and rays of every polytope {theta : E theta <= f} of the stacked [f | E] rows (CSR by row_off).
    Returns (status [P] int32, n_vert [P], n_ray [P], vertices [V, n_t], incidence [V, 4] uint64, rays [R, n_t], stats dict).  The
    outputs are sized by a first guess; when they do not fit, the call is repeated once with the sizes the library reported."""
    L = load()
    off = numpy.ascontiguousarray(row_off, dtype=numpy.int64).reshape(-1)
    ef = _f64(numpy.asarray(ef_rows, dtype=numpy.float64).reshape(-1, int(n_t) + 1))
    P = len(off) - 1
    status, nv, nr = numpy.zeros(P, dtype=numpy.int32), numpy.zeros(P, dtype=numpy.int64), numpy.zeros(P, dtype=numpy.int64)
    vcap, rcap = 16 * P + 64, 64
    for _ in range(2):
        vert, inc, rays = numpy.empty((vcap, n_t)), numpy.empty((vcap, 4), dtype=numpy.uint64), numpy.empty((rcap, n_t))
        vc, rc_ = ctypes.c_int64(vcap), ctypes.c_int64(rcap)
        st = VertexStats()
        rc = L.mpc_region_vertices(int(device), int(n_t), P, off.ctypes.data_as(_lp), ef.ctypes.data_as(_dp), float(tol), int(slab), int(max_slab),
                                   int(budget), ctypes.byref(vc), ctypes.byref(rc_), status.ctypes.data_as(_ip), nv.ctypes.data_as(_lp),
                                   nr.ctypes.data_as(_lp), vert.ctypes.data_as(_dp), inc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                   rays.ctypes.data_as(_dp), ctypes.byref(st))
        if rc == MPC_ERR_CAPACITY:
            vcap, rcap = int(vc.value), int(rc_.value)
            continue
        if rc != MPC_OK:
            raise MpcError(f'mpc_region_vertices failed ({rc}): {L.mpc_last_global_error().decode()}')
        stats = {name: getattr(st, name) for name, _ in VertexStats._fields_}
        return status, nv, nr, vert[:vc.value], inc[:vc.value], rays[:rc_.value], stats
    raise MpcError('mpc_region_vertices: the outputs did not fit the sizes it reported')


def _region_walk(name, row_off, ef_rows, n_t, vert_off, vertices, incidence, vx_status, tol, max_simplices, budget, device):
    """mpc_region_volumes or mpc_region_moments (``name``): (volume, centroid, second_moment or None, simplices, status, stats)."""
    L = load()
    off = numpy.ascontiguousarray(row_off, dtype=numpy.int64).reshape(-1)
    ef = _f64(numpy.asarray(ef_rows, dtype=numpy.float64).reshape(-1, int(n_t) + 1))
    voff = numpy.ascontiguousarray(vert_off, dtype=numpy.int64).reshape(-1)
    vert = _f64(numpy.asarray(vertices, dtype=numpy.float64).reshape(-1, int(n_t)))
    inc = numpy.ascontiguousarray(incidence, dtype=numpy.uint64).reshape(-1, 4)
    vst = numpy.ascontiguousarray(vx_status, dtype=numpy.int32).reshape(-1)
    P = len(off) - 1
    if len(voff) != P + 1 or len(vst) != P or len(vert) != len(inc) or (P and (int(voff[-1]) != len(vert) or int(off[-1]) != len(ef))):
        raise MpcError(f'{name}: the offsets, statuses, vertices and incidence do not belong together')
    volume, centroid = numpy.empty(P), numpy.empty((P, int(n_t)))
    simplices, status = numpy.zeros(P, dtype=numpy.int64), numpy.zeros(P, dtype=numpy.int32)
    st = VolumeStats()
    m2 = numpy.empty((P, int(n_t), int(n_t))) if name == 'mpc_region_moments' else None
    args = [int(device), int(n_t), P, off.ctypes.data_as(_lp), ef.ctypes.data_as(_dp), voff.ctypes.data_as(_lp), vert.ctypes.data_as(_dp),
            inc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), vst.ctypes.data_as(_ip), float(tol), int(max_simplices), int(budget),
            volume.ctypes.data_as(_dp), centroid.ctypes.data_as(_dp), simplices.ctypes.data_as(_lp), status.ctypes.data_as(_ip)]
    if m2 is not None:
        args.append(m2.ctypes.data_as(_dp))
    rc = getattr(L, name)(*args, ctypes.byref(st))
    if rc != MPC_OK:
        raise MpcError(f'{name} failed ({rc}): {L.mpc_last_global_error().decode()}')
    stats = {'ms': float(st.ms), 'simplices': int(st.simplices), 'max_simplices': int(st.max_simplices), 'launches': int(st.launches),
             'status_counts': [int(v) for v in st.status_counts]}
    return volume, centroid, m2, simplices, status, stats


def region_volumes(row_off, ef_rows, n_t: int, vert_off, vertices, incidence, vx_status, tol: float = 1e-9,
                   max_simplices: int = VOL_DEFAULT_MAX_SIMPLICES, budget: int = 0, device: int = 0):
    """mpc_region_volumes: the volume and centroid of every polytope of the stacked [f | E] rows from the vertices, incidence masks and
    statuses mpc_region_vertices returned for them (vert_off [P + 1] into vertices).  Returns (volume [P], centroid [P, n_t],
    simplices [P] int64, status [P] int32, stats dict)."""
    volume, centroid, _, simplices, status, stats = _region_walk('mpc_region_volumes', row_off, ef_rows, n_t, vert_off, vertices, incidence,
                                                                 vx_status, tol, max_simplices, budget, device)
    return volume, centroid, simplices, status, stats


def region_moments(row_off, ef_rows, n_t: int, vert_off, vertices, incidence, vx_status, tol: float = 1e-9,
                   max_simplices: int = VOL_DEFAULT_MAX_SIMPLICES, budget: int = 0, device: int = 0):
    """mpc_region_moments: region_volumes with the second moment of every polytope.  Returns (volume [P], centroid [P, n_t],
    second_moment [P, n_t, n_t], simplices [P] int64, status [P] int32, stats dict)."""
    return _region_walk('mpc_region_moments', row_off, ef_rows, n_t, vert_off, vertices, incidence, vx_status, tol, max_simplices, budget,
                        device)


def _slice_rows(who, row_off, ef_rows, n, eps):
    """(row_off, ef_rows) checked against the limits of the slice kernels; MpcError before any launch."""
    off = numpy.ascontiguousarray(row_off, dtype=numpy.int64).reshape(-1)
    ef = _f64(numpy.asarray(ef_rows, dtype=numpy.float64))
    if len(off) < 1 or off[0] != 0 or numpy.any(numpy.diff(off) < 0):
        raise MpcError(f'{who}: row_off must start at 0 and not decrease')
    if not 1 <= n <= HR_MAX_DIM:
        raise MpcError(f'{who}: dimension {n} outside 1..{HR_MAX_DIM}')
    if ef.ndim != 2 or ef.shape != (int(off[-1]), n + 1):
        raise MpcError(f'{who}: ef_rows has shape {ef.shape}, expected ({int(off[-1])}, {n + 1})')
    if numpy.any(numpy.diff(off) > HR_MAX_ROWS):
        raise MpcError(f'{who}: at most {HR_MAX_ROWS} rows per region, got {int(numpy.max(numpy.diff(off)))}')
    if not 0.0 < float(eps) < 1.0:
        raise MpcError(f'{who}: eps must lie in (0, 1)')
    return off, ef


def slice_polygons(row_off, ef_rows, theta_0, U, box, eps: float = SLICE_EPS, device: int = 0):
    """The slice of every region {E theta <= f} by the plane theta = theta_0 + U z, clipped to box = (lo0, lo1, hi0, hi1), as a convex
    polygon (include/mpcombi.h, mpc_slice_polygons).  ef_rows [rows, n+1] = [f | E] stacked, row_off [R+1], theta_0 [n],
    U [n, 2].  Returns (vert [rows + 4R, 2], edge_row [rows + 4R], count [R], area [R], status [R]); region r's vertices are
    vert[row_off[r] + 4r :][:count[r]].  The kernel time is left in ``slice_polygons.last_ms``.  Bad shapes, more than 256 rows in a
    region, n outside 1..64 or a box that is not finite with lo < hi raise MpcError before any launch."""
    th0 = _f64(numpy.asarray(theta_0, dtype=numpy.float64).reshape(-1))
    n = len(th0)
    Um = _f64(numpy.asarray(U, dtype=numpy.float64))
    if Um.shape != (n, 2):
        raise MpcError(f'slice_polygons: U has shape {Um.shape}, expected ({n}, 2)')
    bx = _f64(numpy.asarray(box, dtype=numpy.float64).reshape(-1))
    if bx.shape != (4,) or not numpy.all(numpy.isfinite(bx)) or not (bx[0] < bx[2] and bx[1] < bx[3]):
        raise MpcError(f'slice_polygons: box must be (lo0, lo1, hi0, hi1), finite, with lo < hi; got {bx}')
    if not numpy.all(numpy.isfinite(th0)) or not numpy.all(numpy.isfinite(Um)):
        raise MpcError('slice_polygons: theta_0 and U must be finite')
    off, ef = _slice_rows('slice_polygons', row_off, ef_rows, n, eps)
    R = len(off) - 1
    slots = int(off[-1]) + 4 * R
    vert = numpy.zeros((slots, 2))
    edge = numpy.zeros(slots, dtype=numpy.int32)
    count = numpy.zeros(R, dtype=numpy.int32)
    area = numpy.zeros(R)
    status = numpy.zeros(R, dtype=numpy.int32)
    ms = ctypes.c_float(0.0)
    L = load()
    rc = L.mpc_slice_polygons(int(device), n, R, off.ctypes.data_as(_lp), ef.ctypes.data_as(_dp), th0.ctypes.data_as(_dp), Um.ctypes.data_as(_dp),
                              bx.ctypes.data_as(_dp), float(eps), vert.ctypes.data_as(_dp), edge.ctypes.data_as(_ip), count.ctypes.data_as(_ip),
                              area.ctypes.data_as(_dp), status.ctypes.data_as(_ip), ctypes.byref(ms))
    if rc != MPC_OK:
        raise MpcError(f'mpc_slice_polygons failed ({rc}): {L.mpc_last_global_error().decode()}')
    slice_polygons.last_ms = float(ms.value)
    return vert, edge, count, area, status


slice_polygons.last_ms = 0.0


def slice_intervals(row_off, ef_rows, theta_0, u, t_range, eps: float = SLICE_EPS, device: int = 0):
    """The slice of every region by the line theta = theta_0 + u t within t_range = (t_lo, t_hi) (mpc_slice_intervals): (interval [R, 2]
    (NaN rows for MPC_SLICE_EMPTY), status [R]).  The kernel time is left in ``slice_intervals.last_ms``; MpcError before any launch
    for bad inputs."""
    th0 = _f64(numpy.asarray(theta_0, dtype=numpy.float64).reshape(-1))
    n = len(th0)
    uv = _f64(numpy.asarray(u, dtype=numpy.float64).reshape(-1))
    if uv.shape != (n,) or not numpy.all(numpy.isfinite(uv)) or not numpy.all(numpy.isfinite(th0)):
        raise MpcError(f'slice_intervals: theta_0 and u must be finite vectors of the same length, got {th0.shape} and {uv.shape}')
    t_lo, t_hi = (float(v) for v in t_range)
    if not (numpy.isfinite(t_lo) and numpy.isfinite(t_hi) and t_lo < t_hi):
        raise MpcError(f'slice_intervals: t_range must be finite with t_lo < t_hi, got {(t_lo, t_hi)}')
    off, ef = _slice_rows('slice_intervals', row_off, ef_rows, n, eps)
    R = len(off) - 1
    interval = numpy.zeros((R, 2))
    status = numpy.zeros(R, dtype=numpy.int32)
    ms = ctypes.c_float(0.0)
    L = load()
    rc = L.mpc_slice_intervals(int(device), n, R, off.ctypes.data_as(_lp), ef.ctypes.data_as(_dp), th0.ctypes.data_as(_dp), uv.ctypes.data_as(_dp),
                               t_lo, t_hi, float(eps), interval.ctypes.data_as(_dp), status.ctypes.data_as(_ip), ctypes.byref(ms))
    if rc != MPC_OK:
        raise MpcError(f'mpc_slice_intervals failed ({rc}): {L.mpc_last_global_error().decode()}')
    slice_intervals.last_ms = float(ms.value)
    return interval, status


slice_intervals.last_ms = 0.0


def facet_centres(ef_rows: numpy.ndarray, row_off: numpy.ndarray, device: int = 0):
    """Chebyshev centre [R, n_t], radius [R] and LP status [R] of every facet (row) of the stacked polytopes
    (include/mpcombi.h, mpc_facet_centres)."""
    L = load()
    ef = _f64(ef_rows)
    off = numpy.ascontiguousarray(row_off, dtype=numpy.int64)
    R, n_t = len(ef), ef.shape[1] - 1
    centre, radius, status = numpy.zeros((R, n_t)), numpy.zeros(R), numpy.zeros(R, dtype=numpy.int32)
    rc = L.mpc_facet_centres(int(device), n_t, len(off) - 1, off.ctypes.data_as(_lp), ef.ctypes.data_as(_dp), centre.ctypes.data_as(_dp),
                             radius.ctypes.data_as(_dp), status.ctypes.data_as(_ip))
    if rc != MPC_OK:
        raise MpcError(f'mpc_facet_centres failed ({rc}): {L.mpc_last_global_error().decode()}')
    return centre, radius, status


MERGE_MAX_ROWS = 256   # rows per region of mpc_merge_regions / mpc_merge_pairs (include/mpcombi.h)
MERGE_WORDS = 4        # 64-bit words of a row mask (MPC_MERGE_WORDS)


def _merge_rows(who, row_off, ef_rows):
    off = numpy.ascontiguousarray(row_off, dtype=numpy.int64).reshape(-1)
    ef = _f64(numpy.asarray(ef_rows, dtype=numpy.float64))
    if ef.ndim != 2 or len(off) < 1 or off[0] != 0 or off[-1] != len(ef):
        raise MpcError(f'{who}: row_off [n_regions + 1] must run from 0 to the number of rows of ef_rows [rows, n_t + 1]')
    return off, ef


_PTR = {numpy.dtype(numpy.float64): _dp, numpy.dtype(numpy.int64): _lp, numpy.dtype(numpy.int32): _ip, numpy.dtype(numpy.uint64): _u64p,
        numpy.dtype(numpy.uint8): _u8p}


def _ptr(a):
    """the ctypes pointer of an array by its dtype; None (an optional array left out) stays None"""
    return None if a is None else a.ctypes.data_as(_PTR[a.dtype])


def _index_arrays(who, names, *arrays):
    """int32 index vectors of one length; ``names`` words the refusal"""
    out = [numpy.ascontiguousarray(a, dtype=numpy.int32).reshape(-1) for a in arrays]
    if any(a.shape != out[0].shape for a in out):
        raise MpcError(f'{who}: {names} must have the same length')
    return out


def _geometry_call(name, keys, *args):
    """One call of the merge / overlap / transition / exit family: L.<name>(*args, stats, ms), arrays (and None) passed as pointers.
    The stats dict, the counters under ``keys`` and the device time under 'ms'; MpcError with the library's message when it refuses."""
    L = load()
    st, ms = numpy.zeros(len(keys), dtype=numpy.int64), ctypes.c_float(0.0)
    rc = getattr(L, name)(*[_ptr(a) if a is None or isinstance(a, numpy.ndarray) else a for a in args], _ptr(st), ctypes.byref(ms))
    if rc != MPC_OK:
        raise MpcError(f'{name} failed ({rc}): {L.mpc_last_error(None).decode()}')
    return dict({k: int(v) for k, v in zip(keys, st)}, ms=float(ms.value))


def merge_regions(row_off, ef_rows, device: int = 0):
    """(xs [R, n_t] a feasible point, box [R, 2, n_t] lower / upper bounds, status [R] (1: empty), stats) of every region of unit rows
    ef_rows = [o | n] (include/mpcombi.h, mpc_merge_regions).  The limits are checked by the library before any launch (MpcError)."""
    off, ef = _merge_rows('merge_regions', row_off, ef_rows)
    n_t, R = ef.shape[1] - 1, len(off) - 1
    xs, box, status = numpy.zeros((R, n_t)), numpy.zeros((R, 2, n_t)), numpy.zeros(R, dtype=numpy.int32)
    stats = _geometry_call('mpc_merge_regions', ('lps', 'pivots', 'capped'), int(device), n_t, R, off, ef, xs, box, status)
    return xs, box, status, stats


def merge_pairs(row_off, ef_rows, xs, box, pair_a, pair_b, tol: float, device: int = 0):
    """The convexity test of every pair of regions (include/mpcombi.h, mpc_merge_pairs): (env_a [n_pairs, MERGE_WORDS] uint64,
    env_b, verdict [n_pairs] int32, t_max [n_pairs], stats)."""
    off, ef = _merge_rows('merge_pairs', row_off, ef_rows)
    n_t, R = ef.shape[1] - 1, len(off) - 1
    x = _f64(numpy.asarray(xs, dtype=numpy.float64)).reshape(R, n_t)
    bx = _f64(numpy.asarray(box, dtype=numpy.float64)).reshape(R, 2, n_t)
    pa, pb = _index_arrays('merge_pairs', 'pair_a and pair_b', pair_a, pair_b)
    n = len(pa)
    env_a, env_b = numpy.zeros((n, MERGE_WORDS), dtype=numpy.uint64), numpy.zeros((n, MERGE_WORDS), dtype=numpy.uint64)
    verdict, t_max = numpy.zeros(n, dtype=numpy.int32), numpy.zeros(n)
    stats = _geometry_call('mpc_merge_pairs', ('pairs', 'box_pairs', 'rows', 'box_rows', 'lps', 'pivots', 'capped'), int(device), n_t, R, off, ef, x, bx,
                           n, pa, pb, float(tol), env_a, env_b, verdict, t_max)
    return env_a, env_b, verdict, t_max, stats


OVERLAP_MEETS, OVERLAP_CUT_ROW, OVERLAP_WIDE = 1, 2, 4   # flag bits of mpc_overlap_split (include/mpcombi.h)


def _cut_rows(who, n, n_t, has_cut, cut_rows):
    hc = numpy.ascontiguousarray(has_cut, dtype=numpy.int32).reshape(-1)
    if len(hc) != n:
        raise MpcError(f'{who}: has_cut must have one entry per item')
    cut = None
    if cut_rows is not None:
        cut = _f64(numpy.asarray(cut_rows, dtype=numpy.float64)).reshape(-1, n_t + 1)
        if len(cut) != n:
            raise MpcError(f'{who}: cut_rows must be [items, n_t + 1]')
    return hc, cut


def _pieces(who, row_off, ef_rows, piece_off, piece_rows):
    """the regions and the pieces of a split call: (off, ef, poff, pef, n_t)"""
    off, ef = _merge_rows(who, row_off, ef_rows)
    poff, pef = _merge_rows(who, piece_off, piece_rows)
    if pef.shape[1] != ef.shape[1]:
        raise MpcError(f'{who}: regions and pieces must have the same n_t')
    return off, ef, poff, pef, ef.shape[1] - 1


_SPLIT_KEYS = ('items', 'meets', 'lps', 'pivots', 'wide')


def overlap_pairs(row_off, ef_rows, xs, pair_a, pair_b, has_cut, cut_rows, tol: float, device: int = 0):
    """The pair stage of the overlap removal (include/mpcombi.h, mpc_overlap_pairs): (radius [n_pairs], d_min, d_max, flag int32, stats)."""
    off, ef = _merge_rows('overlap_pairs', row_off, ef_rows)
    n_t, R = ef.shape[1] - 1, len(off) - 1
    x = _f64(numpy.asarray(xs, dtype=numpy.float64)).reshape(R, n_t)
    pa, pb = _index_arrays('overlap_pairs', 'pair_a and pair_b', pair_a, pair_b)
    n = len(pa)
    hc, cut = _cut_rows('overlap_pairs', n, n_t, has_cut, cut_rows)
    radius, d_min, d_max, flag = numpy.zeros(n), numpy.zeros(n), numpy.zeros(n), numpy.zeros(n, dtype=numpy.int32)
    stats = _geometry_call('mpc_overlap_pairs', ('pairs', 'lps', 'pivots', 'capped'), int(device), n_t, R, off, ef, x, n, pa, pb, hc, cut, float(tol),
                           radius, d_min, d_max, flag)
    return radius, d_min, d_max, flag, stats


LAW_GAP_KEYS = ('pairs', 'meets', 'constant_rows', 'lps', 'pivots', 'wide')


def law_gap_pairs(row_off, ef_rows, laws, xs, pair_a, pair_b, tol: float, ranges: bool = False, device: int = 0):
    """The largest law gap of every pair of regions (include/mpcombi.h, mpc_law_gap_pairs): laws [R, n_out, n_t + 1] = [b | A];
    (radius [n_pairs], gap, gap_row int32, witness [n_pairs, n_t], range [n_pairs, n_out, 2] or None, flag int32, stats)."""
    off, ef = _merge_rows('law_gap_pairs', row_off, ef_rows)
    n_t, R = ef.shape[1] - 1, len(off) - 1
    lw = _f64(numpy.asarray(laws, dtype=numpy.float64))
    if lw.ndim != 3 or lw.shape[0] != R or lw.shape[2] != n_t + 1:
        raise MpcError('law_gap_pairs: laws must be [regions, n_out, n_t + 1]')
    n_out = lw.shape[1]
    x = _f64(numpy.asarray(xs, dtype=numpy.float64)).reshape(R, n_t)
    pa, pb = _index_arrays('law_gap_pairs', 'pair_a and pair_b', pair_a, pair_b)
    n = len(pa)
    radius, gap, row, witness = numpy.zeros(n), numpy.zeros(n), numpy.zeros(n, dtype=numpy.int32), numpy.zeros((n, n_t))
    rng = numpy.zeros((n, n_out, 2)) if ranges else None
    flag = numpy.zeros(n, dtype=numpy.int32)
    stats = _geometry_call('mpc_law_gap_pairs', LAW_GAP_KEYS, int(device), n_t, n_out, R, off, ef, lw, x, n, pa, pb, float(tol), radius, gap, row,
                           witness, rng, flag)
    return radius, gap, row, witness, rng, flag, stats


BOX_CROSS, BOX_UPPER = 0, 1               # mode of mpc_box_pairs (include/mpcombi.h)
SCREEN_ROWS_A, SCREEN_ROWS_B = 1, 2       # sides of mpc_pair_screen
BOX_PAIR_KEYS = ('tests', 'pairs', 'segments')
PAIR_SCREEN_KEYS = ('pairs', 'dropped', 'rows_read')


def _boxes(who, box, usable):
    """a family of mpc_box_pairs: (box [R, 2, n_t] float64, usable [R] uint8), or (None, None) for a family left out"""
    if box is None:
        return None, None
    b = _f64(numpy.asarray(box, dtype=numpy.float64))
    u = numpy.ascontiguousarray(numpy.asarray(usable).reshape(-1) != 0, dtype=numpy.uint8)
    if b.ndim != 3 or b.shape[1] != 2 or len(u) != len(b):
        raise MpcError(f'{who}: boxes must be [R, 2, n_t] with one usable entry per box')
    return b, u


def box_pairs(box_a, usable_a, box_b, usable_b, margin: float, i0: int, i1: int, cap: int, pair_a=None, pair_b=None, row_counts: bool = False,
              device: int = 0):
    """The candidate sweep (include/mpcombi.h, mpc_box_pairs): family b None is BOX_UPPER.  ``pair_a``, ``pair_b``: int64 arrays of at
    least ``cap`` entries to write into (made here when None and cap > 0).  (total, pair_a, pair_b, row_count or None, stats): the
    arrays as given, filled with the ``total`` pairs iff 0 < total <= cap and untouched otherwise."""
    who = 'box_pairs'
    ba, ua = _boxes(who, box_a, usable_a)
    bb, ub = _boxes(who, box_b, usable_b)
    if ba is None:
        raise MpcError(f'{who}: family a is missing')
    if bb is not None and bb.shape[2] != ba.shape[2]:
        raise MpcError(f'{who}: the two families must have the same n_t')
    cap = int(cap)
    if cap > 0:
        pair_a = numpy.zeros(cap, dtype=numpy.int64) if pair_a is None else pair_a
        pair_b = numpy.zeros(cap, dtype=numpy.int64) if pair_b is None else pair_b
        for p in (pair_a, pair_b):
            if not (isinstance(p, numpy.ndarray) and p.dtype == numpy.int64 and p.ndim == 1 and len(p) >= cap and p.flags.c_contiguous):
                raise MpcError(f'{who}: pair_a and pair_b must be contiguous int64 arrays of at least cap entries')
    rc = numpy.zeros(max(int(i1) - int(i0), 0), dtype=numpy.int64) if row_counts else None
    total = numpy.zeros(1, dtype=numpy.int64)
    stats = _geometry_call('mpc_box_pairs', BOX_PAIR_KEYS, int(device), ba.shape[2], BOX_UPPER if bb is None else BOX_CROSS, len(ba), ba, ua,
                           0 if bb is None else len(bb), bb, ub, float(margin), int(i0), int(i1), cap, pair_a if cap > 0 else None,
                           pair_b if cap > 0 else None, rc, total)
    return int(total[0]), pair_a, pair_b, rc, stats


def pair_screen(row_off, ef_rows, pair_a, pair_b, box_for_a_rows, box_for_b_rows, sides: int, device: int = 0):
    """The row screen of a candidate list (include/mpcombi.h, mpc_pair_screen): (keep [n_pairs] uint8, stats)."""
    who = 'pair_screen'
    off, ef = _merge_rows(who, row_off, ef_rows)
    n_t, R = ef.shape[1] - 1, len(off) - 1
    pa = numpy.ascontiguousarray(pair_a, dtype=numpy.int64).reshape(-1)
    pb = numpy.ascontiguousarray(pair_b, dtype=numpy.int64).reshape(-1)
    if pa.shape != pb.shape:
        raise MpcError(f'{who}: pair_a and pair_b must have the same length')
    boxes = []
    for b in (box_for_a_rows, box_for_b_rows):
        if b is not None:
            b = _f64(numpy.asarray(b, dtype=numpy.float64))
            if b.shape != (R, 2, n_t):
                raise MpcError(f'{who}: a box table must be [regions, 2, n_t]')
        boxes.append(b)
    keep = numpy.ones(len(pa), dtype=numpy.uint8)
    stats = _geometry_call('mpc_pair_screen', PAIR_SCREEN_KEYS, int(device), n_t, R, off, ef, len(pa), pa, pb, boxes[0], boxes[1], int(sides), keep)
    return keep, stats


def overlap_split(row_off, ef_rows, piece_off, piece_rows, item_piece, item_cutter, has_cut, cut_rows, start, tol: float, device: int = 0):
    """One round of the region difference (include/mpcombi.h, mpc_overlap_split): (flag [n_items] int32, mask [n_items, MERGE_WORDS]
    uint64, stats)."""
    off, ef, poff, pef, n_t = _pieces('overlap_split', row_off, ef_rows, piece_off, piece_rows)
    ip, ic = _index_arrays('overlap_split', 'item_piece and item_cutter', item_piece, item_cutter)
    n = len(ip)
    hc, cut = _cut_rows('overlap_split', n, n_t, has_cut, cut_rows)
    s0 = None if start is None else _f64(numpy.asarray(start, dtype=numpy.float64)).reshape(n, n_t)
    flag, mask = numpy.zeros(n, dtype=numpy.int32), numpy.zeros((n, MERGE_WORDS), dtype=numpy.uint64)
    stats = _geometry_call('mpc_overlap_split', _SPLIT_KEYS, int(device), n_t, len(off) - 1, off, ef, len(poff) - 1, poff, pef, n, ip, ic, hc, cut, s0,
                           float(tol), flag, mask)
    return flag, mask, stats


TRANSITION_NO_EDGE, TRANSITION_EDGE, TRANSITION_UNBOUNDED, TRANSITION_UNDECIDED = range(4)   # status of mpc_transition_pairs (include/mpcombi.h)


def _transition_maps(who, R, n_t, Phi, phi, xs):
    P = _f64(numpy.asarray(Phi, dtype=numpy.float64))
    p = _f64(numpy.asarray(phi, dtype=numpy.float64))
    x = _f64(numpy.asarray(xs, dtype=numpy.float64))
    if P.size != R * n_t * n_t or p.size != R * n_t or x.size != R * n_t:
        raise MpcError(f'{who}: Phi must be [regions, n_t, n_t], phi and xs [regions, n_t]')
    return P.reshape(R, n_t, n_t), p.reshape(R, n_t), x.reshape(R, n_t)


def transition_boxes(row_off, ef_rows, Phi, phi, xs, device: int = 0):
    """The bounding boxes of the images Phi_i R_i + phi_i (include/mpcombi.h, mpc_transition_boxes): (image_box [R, 2, n_t] lower /
    upper bounds, flag [R] int32 (1: a run was capped), stats)."""
    off, ef = _merge_rows('transition_boxes', row_off, ef_rows)
    n_t, R = ef.shape[1] - 1, len(off) - 1
    P, p, x = _transition_maps('transition_boxes', R, n_t, Phi, phi, xs)
    box, flag = numpy.zeros((R, 2, n_t)), numpy.zeros(R, dtype=numpy.int32)
    stats = _geometry_call('mpc_transition_boxes', ('lps', 'pivots', 'capped'), int(device), n_t, R, off, ef, P, p, x, box, flag)
    return box, flag, stats


def transition_pairs(row_off, ef_rows, Phi, phi, xs, pair_a, pair_b, full_radius: bool, tol: float, device: int = 0):
    """The pair stage of the transition graph (include/mpcombi.h, mpc_transition_pairs): (radius [n_pairs], status int32, witness
    [n_pairs, n_t], stats)."""
    off, ef = _merge_rows('transition_pairs', row_off, ef_rows)
    n_t, R = ef.shape[1] - 1, len(off) - 1
    P, p, x = _transition_maps('transition_pairs', R, n_t, Phi, phi, xs)
    pa, pb = _index_arrays('transition_pairs', 'pair_a and pair_b', pair_a, pair_b)
    n = len(pa)
    radius, status, witness = numpy.zeros(n), numpy.zeros(n, dtype=numpy.int32), numpy.zeros((n, n_t))
    stats = _geometry_call('mpc_transition_pairs', ('pairs', 'lps', 'pivots', 'capped'), int(device), n_t, R, off, ef, P, p, x, n, pa, pb,
                           1 if full_radius else 0, float(tol), radius, status, witness)
    return radius, status, witness, stats


def exit_split(row_off, ef_rows, Phi, phi, piece_off, piece_rows, item_piece, item_source, item_target, start, tol: float, device: int = 0):
    """One round of the region difference against pulled-back cutters (include/mpcombi.h, mpc_exit_split): (flag [n_items] int32 with the
    bits OVERLAP_MEETS and OVERLAP_WIDE, mask [n_items, MERGE_WORDS] uint64, stats)."""
    off, ef, poff, pef, n_t = _pieces('exit_split', row_off, ef_rows, piece_off, piece_rows)
    R = len(off) - 1
    M = _f64(numpy.asarray(Phi, dtype=numpy.float64))
    p = _f64(numpy.asarray(phi, dtype=numpy.float64))
    if M.size != R * n_t * n_t or p.size != R * n_t:
        raise MpcError('exit_split: Phi must be [regions, n_t, n_t] and phi [regions, n_t]')
    ip, src, dst = _index_arrays('exit_split', 'item_piece, item_source and item_target', item_piece, item_source, item_target)
    n = len(ip)
    s0 = None if start is None else _f64(numpy.asarray(start, dtype=numpy.float64)).reshape(n, n_t)
    flag, mask = numpy.zeros(n, dtype=numpy.int32), numpy.zeros((n, MERGE_WORDS), dtype=numpy.uint64)
    stats = _geometry_call('mpc_exit_split', _SPLIT_KEYS, int(device), n_t, R, off, ef, M, p, len(poff) - 1, poff, pef, n, ip, src, dst, s0, float(tol),
                           flag, mask)
    return flag, mask, stats


REDUCE_MAX_ROWS = 512   # rows per polytope of mpc_reduce_rows (include/mpcombi.h)
REDUCE_WORDS = 8        # 64-bit words of its kept mask (MPC_REDUCE_WORDS)
REDUCE_OK, REDUCE_THIN = 0, 1


def reduce_rows(row_off, ef_rows, start, tol: float, device: int = 0):
    """The redundant rows of every polytope by the sequential rule (include/mpcombi.h, mpc_reduce_rows): (kept [rows] bool, one per input
    row, status [n_poly] int32 (REDUCE_OK, REDUCE_THIN), wide [n_poly] int32, point [n_poly, n_t], stats)."""
    off, ef = _merge_rows('reduce_rows', row_off, ef_rows)
    n_t, n = ef.shape[1] - 1, len(off) - 1
    s0 = None if start is None else _f64(numpy.asarray(start, dtype=numpy.float64)).reshape(n, n_t)
    status, wide, mask = numpy.zeros(n, dtype=numpy.int32), numpy.zeros(n, dtype=numpy.int32), numpy.zeros((n, REDUCE_WORDS), dtype=numpy.uint64)
    point = numpy.zeros((n, n_t))
    stats = _geometry_call('mpc_reduce_rows', ('polytopes', 'thin', 'lps', 'pivots', 'wide'), int(device), n_t, n, off, ef, s0, float(tol), status,
                           wide, mask, point)
    counts = numpy.diff(off)
    poly = numpy.repeat(numpy.arange(n), counts)
    k = numpy.arange(len(ef)) - numpy.repeat(off[:-1], counts)
    kept = ((mask[poly, k >> 6] >> (k & 63).astype(numpy.uint64)) & numpy.uint64(1)).astype(bool)
    return kept, status, wide, point, stats


SUPPORT_MAX_ROWS = 512   # rows per polytope of mpc_support_rows (include/mpcombi.h)
SUPPORT_OK, SUPPORT_UNBOUNDED, SUPPORT_CAPPED, SUPPORT_THIN = range(4)
SUPPORT_STATUS = ('OK', 'UNBOUNDED', 'CAPPED', 'THIN')


def support_rows(row_off, ef_rows, dir_off, dirs, start, tol: float, args: bool = True, device: int = 0):
    """h_P(d) for every polytope and each of its directions (include/mpcombi.h, mpc_support_rows): (value [n_dir], arg [n_dir, n_t] or None
    without ``args``, dir_status [n_dir] int32 (SUPPORT_*), poly_status [n_poly] int32 (SUPPORT_OK, SUPPORT_THIN), wide [n_poly] int32,
    point [n_poly, n_t], stats).  Polytope q owns the rows dir_off[q] .. dir_off[q + 1] of dirs."""
    off, ef = _merge_rows('support_rows', row_off, ef_rows)
    n_t, n = ef.shape[1] - 1, len(off) - 1
    doff = numpy.ascontiguousarray(dir_off, dtype=numpy.int64).reshape(-1)
    d = _f64(numpy.asarray(dirs, dtype=numpy.float64)).reshape(-1, n_t)
    if len(doff) != n + 1 or doff[-1] != len(d):
        raise MpcError('support_rows: dir_off [n_poly + 1] must end at the number of rows of dirs [n_dir, n_t]')
    s0 = None if start is None else _f64(numpy.asarray(start, dtype=numpy.float64)).reshape(n, n_t)
    value, arg, ds = numpy.zeros(len(d)), (numpy.zeros((len(d), n_t)) if args else None), numpy.zeros(len(d), dtype=numpy.int32)
    ps, wide, point = numpy.zeros(n, dtype=numpy.int32), numpy.zeros(n, dtype=numpy.int32), numpy.zeros((n, n_t))
    stats = _geometry_call('mpc_support_rows', ('polytopes', 'thin', 'directions', 'zero', 'lps', 'pivots', 'wide'), int(device), n_t, n, off, ef,
                           doff, d, s0, float(tol), value, arg, ds, ps, wide, point)
    return value, arg, ds, ps, wide, point, stats


PROJECT_MAX_ROWS = 512   # rows per polytope and per elimination step of mpc_project_rows (include/mpcombi.h)
PROJECT_OK, PROJECT_THIN, PROJECT_WHOLE, PROJECT_TOO_LARGE = range(4)
PROJECT_STATUS = ('OK', 'THIN', 'WHOLE', 'TOO_LARGE')


def project_rows(row_off, ef_rows, n_elim: int, start, tol: float, out_cap: int = PROJECT_MAX_ROWS, device: int = 0):
    """The projections of the polytopes onto their first n - n_elim coordinates (include/mpcombi.h, mpc_project_rows): (out_off
    [n_poly + 1] int64, out_rows [out_off[-1], n - n_elim + 1] unit rows, status [n_poly] int32 (PROJECT_*), wide, peak int32, point
    [n_poly, n - n_elim], stats)."""
    off, ef = _merge_rows('project_rows', row_off, ef_rows)
    n, count = ef.shape[1] - 1, len(off) - 1
    k = n - int(n_elim)
    s0 = None if start is None else _f64(numpy.asarray(start, dtype=numpy.float64)).reshape(count, n)
    cap = int(out_cap)
    rows = numpy.zeros((count, max(cap, 0), max(k, 0) + 1))
    n_out, status, wide, peak = (numpy.zeros(count, dtype=numpy.int32) for _ in range(4))
    point = numpy.zeros((count, max(k, 0)))
    stats = _geometry_call('mpc_project_rows', ('polytopes', 'thin', 'whole', 'too_large', 'steps', 'rows_made', 'lps', 'pivots', 'wide'), int(device),
                           n, int(n_elim), count, off, ef, s0, float(tol), cap, rows, n_out, status, wide, peak, point)
    out_off = numpy.concatenate([[0], numpy.cumsum(n_out, dtype=numpy.int64)]).astype(numpy.int64)
    taken = numpy.arange(cap)[None, :] < n_out[:, None]
    return out_off, rows[taken], status, wide, peak, point, stats


class _CellCall:
    """What backward_exits and forward_cells share around their library call.  The cells of step 0 converted and checked (``per_cell``:
    what the refusal says every cell has one of; n_points: the rows of the caller's point array, None without one) and the limits, then
    capacity-sized outputs, grouped as the C argument lists have them: cells0 (count, cell_off, cell_rows, region), limits (max_steps,
    max_cells, max_rows_total), table (n_cells, cell_off, cell_rows, region, step, parent, wide, point), status, steps, per_step
    (cells_per_step, step_ms)."""

    def __init__(self, who, n_t, cell_off, cell_rows, cell_reg, per_cell, n_points, max_steps, max_cells, max_rows_total):
        coff = numpy.ascontiguousarray(cell_off, dtype=numpy.int64).reshape(-1)
        crow = _f64(numpy.asarray(cell_rows, dtype=numpy.float64)).reshape(-1, n_t + 1)
        creg = numpy.ascontiguousarray(cell_reg, dtype=numpy.int32).reshape(-1)
        if len(coff) != len(creg) + 1 or coff[0] != 0 or coff[-1] != len(crow) or (n_points is not None and n_points != len(creg)):
            raise MpcError(f'{who}: cell_off [cells + 1] must run from 0 to the number of rows of cell_rows, with {per_cell} per cell')
        max_steps, max_cells, max_rows_total = int(max_steps), int(max_cells), int(max_rows_total)
        if max_cells < 0 or max_rows_total < 0:
            raise MpcError(f'{who}: max_cells and max_rows_total must be >= 0')
        self.cells0, self.limits = (len(creg), coff, crow, creg), (max_steps, max_cells, max_rows_total)
        # capacity, not contents: pages the library never writes are never touched
        reg, step, parent, wide = (numpy.empty(max_cells, dtype=numpy.int32) for _ in range(4))
        self.table = (numpy.zeros(1, dtype=numpy.int64), numpy.empty(max_cells + 1, dtype=numpy.int64), numpy.empty((max_rows_total, n_t + 1)),
                      reg, step, parent, wide, numpy.empty((max_cells, n_t)))
        self.status, self.steps = numpy.zeros(1, dtype=numpy.int32), numpy.zeros(1, dtype=numpy.int32)
        self.step_ms = numpy.zeros(max(max_steps, 1), dtype=numpy.float32)
        self.per_step = (numpy.zeros(max(max_steps, 0) + 1, dtype=numpy.int64), self.step_ms.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))

    def result(self, reg_key, stats):
        """The keys both results have (the region of a cell under ``reg_key``), cut to the cells the call delivered."""
        n, out_off, out_rows, reg, step, parent, wide, point = self.table
        n, k = int(n[0]), int(self.steps[0])
        return {'cell_off': out_off[:n + 1].copy(), 'cell_rows': out_rows[:int(out_off[n])].copy(), reg_key: reg[:n].astype(numpy.int64),
                'step': step[:n].astype(numpy.int64), 'parent': parent[:n].astype(numpy.int64), 'wide': wide[:n] != 0, 'point': point[:n].copy(),
                'status': int(self.status[0]), 'steps': k, 'cells_per_step': self.per_step[0][:k + 1].copy(),
                'step_ms': self.step_ms[:max(self.limits[0], 0)].astype(numpy.float64), 'stats': stats}


_CELL_STATS = ('items', 'cells', 'empty', 'lps', 'pivots', 'wide')

# status of mpc_backward_exits (include/mpcombi.h)
BACKWARD_CONVERGED, BACKWARD_MAX_STEPS, BACKWARD_ROWS, BACKWARD_MAX_CELLS, BACKWARD_MAX_ROWS_TOTAL = range(5)
BACKWARD_STATUS = ('CONVERGED', 'MAX_STEPS', 'ROWS', 'MAX_CELLS', 'MAX_ROWS_TOTAL')


def backward_exits(row_off, ef_rows, Phi, phi, xs, pred_off, pred_idx, cell_off, cell_rows, cell_source, tol: float, max_steps: int, max_cells: int,
                   max_rows_total: int, device: int = 0):
    """The backward exit cells of a closed loop, every step in one call (include/mpcombi.h, mpc_backward_exits).  A dict: cell_off,
    cell_rows, source, step, parent, wide (bool), point (NaN rows at step 0), status (BACKWARD_*), steps, converged, cells_per_step
    [steps + 1], step_ms [max_steps] and stats (items, cells, empty, lps, pivots, wide, ms)."""
    who = 'backward_exits'
    off, ef = _merge_rows(who, row_off, ef_rows)
    n_t, R = ef.shape[1] - 1, len(off) - 1
    P, p, x = _transition_maps(who, R, n_t, Phi, phi, xs)
    poff = numpy.ascontiguousarray(pred_off, dtype=numpy.int64).reshape(-1)
    pidx = numpy.ascontiguousarray(pred_idx, dtype=numpy.int32).reshape(-1)
    if len(poff) != R + 1 or (len(poff) and poff[-1] != len(pidx)):
        raise MpcError(f'{who}: pred_off [regions + 1] must end at the length of pred_idx')
    t = _CellCall(who, n_t, cell_off, cell_rows, cell_source, 'one source', None, max_steps, max_cells, max_rows_total)
    conv = numpy.zeros(1, dtype=numpy.int32)
    stats = _geometry_call('mpc_backward_exits', _CELL_STATS, int(device), n_t, R, off, ef, P, p, x, poff, pidx, *t.cells0, float(tol), *t.limits,
                           *t.table, t.status, t.steps, conv, *t.per_step)
    r = t.result('source', stats)
    r['point'][:t.cells0[0]] = numpy.nan
    r['converged'] = bool(conv[0])
    return r


# status of mpc_forward_cells (include/mpcombi.h)
FORWARD_DONE, FORWARD_EMPTY, FORWARD_ROWS, FORWARD_MAX_CELLS, FORWARD_MAX_ROWS_TOTAL = range(5)
FORWARD_STATUS = ('DONE', 'EMPTY', 'ROWS', 'MAX_CELLS', 'MAX_ROWS_TOTAL')


def forward_cells(row_off, ef_rows, Phi, phi, succ_off, succ_idx, cell_off, cell_rows, cell_region, cell_point, tol: float, max_steps: int,
                  max_cells: int, max_rows_total: int, device: int = 0):
    """The forward cells of a closed loop, every step in one call (include/mpcombi.h, mpc_forward_cells).  A dict: cell_off, cell_rows,
    region, step, parent, wide (bool), point, G [cells, n_t, n_t], g [cells, n_t], status (FORWARD_*), steps, cells_per_step [steps + 1],
    step_ms [max_steps] and stats (items, cells, empty, lps, pivots, wide, ms)."""
    who = 'forward_cells'
    off, ef = _merge_rows(who, row_off, ef_rows)
    n_t, R = ef.shape[1] - 1, len(off) - 1
    P = _f64(numpy.asarray(Phi, dtype=numpy.float64))
    p = _f64(numpy.asarray(phi, dtype=numpy.float64))
    if P.size != R * n_t * n_t or p.size != R * n_t:
        raise MpcError(f'{who}: Phi must be [regions, n_t, n_t] and phi [regions, n_t]')
    soff = numpy.ascontiguousarray(succ_off, dtype=numpy.int64).reshape(-1)
    sidx = numpy.ascontiguousarray(succ_idx, dtype=numpy.int32).reshape(-1)
    if len(soff) != R + 1 or (len(soff) and soff[-1] != len(sidx)):
        raise MpcError(f'{who}: succ_off [regions + 1] must end at the length of succ_idx')
    cpt = _f64(numpy.asarray(cell_point, dtype=numpy.float64)).reshape(-1, n_t)
    t = _CellCall(who, n_t, cell_off, cell_rows, cell_region, 'one region and one point', len(cpt), max_steps, max_cells, max_rows_total)
    cmap = numpy.empty((t.limits[1], n_t, n_t + 1))
    stats = _geometry_call('mpc_forward_cells', _CELL_STATS, int(device), n_t, R, off, ef, P, p, soff, sidx, *t.cells0, cpt, float(tol), *t.limits,
                           *t.table, cmap, t.status, t.steps, *t.per_step)
    r = t.result('region', stats)
    n = len(r['region'])
    r['G'], r['g'] = cmap[:n, :, :n_t].copy(), cmap[:n, :, n_t].copy()
    return r


class Locator:
    """Batched point location over stacked critical regions (include/mpcombi.h, mpc_locator_*).
    ef_rows: [total_rows, n_t+1] = [f | E] stacked; row_off: [n_regions+1]; xlaw: [n_regions, n_x, n_t+1] = [b | A]."""

    def __init__(self, row_off, ef_rows, xlaw, Q=None, c=None, H=None, device: int = 0):
        self._L = load()
        self.row_off = numpy.ascontiguousarray(row_off, dtype=numpy.int64)
        self.ef = _f64(ef_rows)
        self.xlaw = _f64(xlaw)
        self.n_regions = len(self.row_off) - 1
        self.n_x, self.n_t = int(self.xlaw.shape[1]), int(self.xlaw.shape[2]) - 1
        opt = [None if a is None else _f64(a) for a in (Q, c, H)]
        self._keep = opt
        ptr = ctypes.c_void_p()
        rc = self._L.mpc_locator_create(device, self.n_x, self.n_t, self.n_regions, self.row_off.ctypes.data_as(_lp),
                                        self.ef.ctypes.data_as(_dp), self.xlaw.ctypes.data_as(_dp),
                                        *[None if a is None else a.ctypes.data_as(_dp) for a in opt], ctypes.byref(ptr))
        if rc != MPC_OK:
            raise MpcError(f'mpc_locator_create failed ({rc}): {self._L.mpc_last_global_error().decode()}')
        self._h = ptr
        self.last_ms = 0.0
        self.has_adjacency = False

    def set_adjacency(self, masks: numpy.ndarray, row_info: numpy.ndarray, n_c: int) -> bool:
        """Facet adjacency for the walk (mpc_locator_set_adjacency): masks [n_regions, words] uint64, row_info [total_rows]
        int32 = kind << 16 | id.  False when the library refuses it (two regions with one active set)."""
        m = numpy.ascontiguousarray(masks, dtype=numpy.uint64)
        ri = numpy.ascontiguousarray(row_info, dtype=numpy.int32)
        rc = self._L.mpc_locator_set_adjacency(self._h, int(m.shape[1]), int(n_c), m.ctypes.data_as(_u64p), ri.ctypes.data_as(_ip))
        self.has_adjacency = rc == MPC_OK
        return self.has_adjacency

    def build_tree(self, planes, cand_off, cand_plane, tol: float, band: float, leaf_size: int = 1, max_depth: int = 48,
                   budget: int = 0) -> dict:
        """Builds a search tree on this locator's rows and attaches it (mpc_tree_build); returns its stats.  planes [H, n_t+1] unit
        [n | o]; cand_off [n_regions+1] / cand_plane: the planes of every region (or both None).  Bad shapes raise MpcError before
        any launch; the library's own limits (rows per region, the bitset budget) raise MpcError with its message."""
        pl = _f64(numpy.asarray(planes, dtype=numpy.float64)).reshape(-1, self.n_t + 1)
        if self.n_t > TREE_MAX_DIM:
            raise MpcError(f'build_tree: n_theta = {self.n_t} > {TREE_MAX_DIM}')
        if not 1 <= int(max_depth) <= TREE_MAX_DEPTH or int(leaf_size) < 1:
            raise MpcError(f'build_tree: max_depth must lie in 1..{TREE_MAX_DEPTH} and leaf_size >= 1')
        if (cand_off is None) != (cand_plane is None):
            raise MpcError('build_tree: cand_off and cand_plane go together')
        co = cp = None
        if cand_off is not None:
            co = numpy.ascontiguousarray(cand_off, dtype=numpy.int64).reshape(-1)
            cp = numpy.ascontiguousarray(cand_plane, dtype=numpy.int32).reshape(-1)
            if len(co) != self.n_regions + 1 or co[0] != 0 or co[-1] != len(cp) or numpy.any(numpy.diff(co) < 0):
                raise MpcError('build_tree: cand_off must hold n_regions + 1 non-decreasing offsets into cand_plane')
            if len(cp) and (cp.min() < 0 or cp.max() >= len(pl)):
                raise MpcError('build_tree: a candidate plane is out of range')
        st = TreeStats()
        rc = self._L.mpc_tree_build(self._h, len(pl), pl.ctypes.data_as(_dp), None if co is None else co.ctypes.data_as(_lp),
                                    None if cp is None else cp.ctypes.data_as(_ip), float(tol), float(band), int(leaf_size), int(max_depth),
                                    int(budget), ctypes.byref(st))
        if rc != MPC_OK:
            raise MpcError(f'mpc_tree_build failed ({rc}): {self._L.mpc_last_global_error().decode()}')
        return st.as_dict()

    def get_tree(self) -> dict:
        """The attached tree's arrays (mpc_locator_get_tree)."""
        n_nodes, n_items, n_planes, tol = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_double()
        rc = self._L.mpc_locator_tree_size(self._h, ctypes.byref(n_nodes), ctypes.byref(n_items), ctypes.byref(n_planes), ctypes.byref(tol))
        if rc != MPC_OK:
            raise MpcError(f'mpc_locator_tree_size failed ({rc}): {self._L.mpc_last_global_error().decode()}')
        N, K, H = n_nodes.value, n_items.value, n_planes.value
        t = {'planes': numpy.zeros((H, self.n_t + 1)), 'node_plane': numpy.zeros(N, dtype=numpy.int32),
             'node_child': numpy.zeros((N, 2), dtype=numpy.int32), 'node_tau': numpy.zeros((N, 2)),
             'node_off': numpy.zeros(N + 1, dtype=numpy.int64), 'items': numpy.zeros(K, dtype=numpy.int32), 'tol': tol.value}
        rc = self._L.mpc_locator_get_tree(self._h, t['planes'].ctypes.data_as(_dp), t['node_plane'].ctypes.data_as(_ip),
                                          t['node_child'].ctypes.data_as(_ip), t['node_tau'].ctypes.data_as(_dp),
                                          t['node_off'].ctypes.data_as(_lp), t['items'].ctypes.data_as(_ip))
        if rc != MPC_OK:
            raise MpcError(f'mpc_locator_get_tree failed ({rc}): {self._L.mpc_last_global_error().decode()}')
        return t

    def set_tree(self, planes, node_plane, node_child, node_tau, node_off, items, tol: float) -> None:
        """Attaches a tree given as arrays (mpc_locator_set_tree); shapes are checked here, contents by the library."""
        pl = _f64(numpy.asarray(planes, dtype=numpy.float64)).reshape(-1, self.n_t + 1)
        npl = numpy.ascontiguousarray(node_plane, dtype=numpy.int32).reshape(-1)
        N = len(npl)
        ch = numpy.ascontiguousarray(node_child, dtype=numpy.int32).reshape(-1)
        tau = _f64(numpy.asarray(node_tau, dtype=numpy.float64)).reshape(-1)
        off = numpy.ascontiguousarray(node_off, dtype=numpy.int64).reshape(-1)
        it = numpy.ascontiguousarray(items, dtype=numpy.int32).reshape(-1)
        if N < 1 or ch.shape != (2 * N,) or tau.shape != (2 * N,) or off.shape != (N + 1,) or off[-1] != len(it):
            raise MpcError('set_tree: node arrays of inconsistent shapes')
        rc = self._L.mpc_locator_set_tree(self._h, len(pl), pl.ctypes.data_as(_dp), N, npl.ctypes.data_as(_ip), ch.ctypes.data_as(_ip),
                                          tau.ctypes.data_as(_dp), off.ctypes.data_as(_lp), it.ctypes.data_as(_ip), float(tol))
        if rc != MPC_OK:
            raise MpcError(f'mpc_locator_set_tree failed ({rc}): {self._L.mpc_last_global_error().decode()}')

    def query(self, theta: numpy.ndarray, tol: float = 1e-5, overlapping: bool = False, want_x: bool = True,
              inclusive: bool = False, walk: bool = False, tree: bool = False):
        """theta [m, n_t] -> (region index [m] (-1: none), x [m, n_x] or None).  ``inclusive``: membership is
        ``E theta <= f + tol`` (MPC_LOCATE_INCLUSIVE) instead of the strict ``E theta - f < tol``."""
        th = _f64(theta).reshape(-1, self.n_t)
        m = len(th)
        region = numpy.empty(m, dtype=numpy.int64)
        x = numpy.empty((m, self.n_x)) if want_x else None
        ms = ctypes.c_float(0.0)
        rc = self._L.mpc_locator_query(self._h, m, th.ctypes.data_as(_dp), float(tol),
                                       (MPC_LOCATE_OVERLAPPING if overlapping else 0) | (MPC_LOCATE_INCLUSIVE if inclusive else 0)
                                       | (MPC_LOCATE_WALK if walk and self.has_adjacency else 0) | (MPC_LOCATE_TREE if tree else 0),
                                       region.ctypes.data_as(_lp), None if x is None else x.ctypes.data_as(_dp), ctypes.byref(ms))
        if rc != MPC_OK:
            raise MpcError(f'mpc_locator_query failed ({rc}): {self._L.mpc_last_global_error().decode()}')
        self.last_ms = float(ms.value)
        return region, x

    @property
    def last_unresolved(self) -> int:
        """Points of the last walk or tree query that went to the exhaustive pass (mpc_locator_last_unresolved)."""
        n = ctypes.c_int64(0)
        rc = self._L.mpc_locator_last_unresolved(self._h, ctypes.byref(n))
        if rc != MPC_OK:
            raise MpcError(f'mpc_locator_last_unresolved failed ({rc})')
        return int(n.value)

    def simulate(self, theta0, steps: int, A, B, inputs, c=None, w=None, box=None, seed: int = 0, tol: float = 1e-5,
                 stop_tol: Optional[float] = None, overlapping: bool = False, inclusive: bool = False, walk: bool = False, tree: bool = False,
                 final_only: bool = False, budget: int = 0):
        """mpc_locator_simulate.  theta0 [n, n_t]; w [steps, n, n_t] step-major or None; box (lo, hi) or None.  Returns the step-major
        arrays (theta [steps+1, n, n_t] or [n, n_t] with final_only, u [steps, n, n_u], region [steps, n] int32 (None with final_only),
        status [n], exit_step [n]) and the stats as a dict."""
        th0 = _f64(theta0).reshape(-1, self.n_t)
        n, steps = len(th0), int(steps)
        A_, B_ = _f64(A).reshape(self.n_t, self.n_t), _f64(B).reshape(self.n_t, -1)
        n_u = B_.shape[1]
        inp = numpy.ascontiguousarray(inputs, dtype=numpy.int32).reshape(-1)
        c_ = None if c is None else _f64(c).reshape(-1)
        w_ = None if w is None else _f64(w).reshape(steps, n, self.n_t)
        lo = hi = None
        if box is not None:
            lo, hi = _f64(box[0]).reshape(-1), _f64(box[1]).reshape(-1)
        theta = numpy.empty((n, self.n_t) if final_only else (steps + 1, n, self.n_t))
        u = None if final_only else numpy.empty((steps, n, n_u))
        region = None if final_only else numpy.empty((steps, n), dtype=numpy.int32)
        status, exit_step = numpy.empty(n, dtype=numpy.int32), numpy.empty(n, dtype=numpy.int32)
        st = SimStats()
        p = lambda a, t=_dp: None if a is None else a.ctypes.data_as(t)
        flags = (MPC_LOCATE_OVERLAPPING if overlapping else 0) | (MPC_LOCATE_INCLUSIVE if inclusive else 0) | (MPC_LOCATE_WALK if walk else 0) \
            | (MPC_LOCATE_TREE if tree else 0) | (MPC_SIM_FINAL if final_only else 0)
        rc = self._L.mpc_locator_simulate(self._h, n, steps, p(th0), n_u, p(inp, _ip), p(A_), p(B_), p(c_), p(w_), p(lo), p(hi), int(seed),
                                          float(tol), -1.0 if stop_tol is None else float(stop_tol), flags, int(budget), p(theta), p(u),
                                          p(region, _ip), p(status, _ip), p(exit_step, _ip), ctypes.byref(st))
        if rc != MPC_OK:
            raise MpcError(f'mpc_locator_simulate failed ({rc}): {self._L.mpc_last_global_error().decode()}')
        stats = {name: getattr(st, name) for name, _ in SimStats._fields_}
        self.last_ms = float(st.ms)
        return theta, u, region, status, exit_step, stats

    def close(self):
        if getattr(self, '_h', None):
            self._L.mpc_locator_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
