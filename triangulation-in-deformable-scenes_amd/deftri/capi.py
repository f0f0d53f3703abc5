"""ctypes binding of libdeftri.so (include/deftri.h).

The library is built in-tree (csrc/Makefile -> triangulation-in-deformable-scenes_amd/libdeftri.so).
There is no CPU fallback: if the library is missing, `load()` raises, and every solve entry
point runs on the GPU or returns an error.
"""
import ctypes as C
import time
import os
import pathlib

import numpy as np

from . import _abi
from .problem import Problem

PKG_ROOT = pathlib.Path(__file__).resolve().parent.parent
LIB_PATH = pathlib.Path(os.environ.get("DEFTRI_LIB", PKG_ROOT / "libdeftri.so"))   # DEFTRI_LIB: dev builds
_lib = None


class DeftriError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"deftri error {code}: {msg}")
        self.code = code


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} not built — run __graft_entry__.build() (make -C csrc)")
    lib = C.CDLL(str(LIB_PATH))
    P = C.POINTER
    sig = {
        "deftri_abi_version": (C.c_int, []),
        "deftri_ctx_create": (C.c_int, [C.c_int32, P(C.c_void_p)]),
        "deftri_ctx_destroy": (C.c_int, [C.c_void_p]),
        "deftri_last_error": (C.c_char_p, [C.c_void_p]),
        "deftri_problem_upload": (C.c_int, [C.c_void_p, P(_abi.ProblemDesc)]),
        "deftri_problem_analyse": (C.c_int, [C.c_void_p, P(_abi.ProblemDesc)]),
        "deftri_plan_stats": (C.c_int, [C.c_void_p, P(_abi.Report)]),
        "deftri_debug_plan_solve": (C.c_int, [C.c_void_p, P(C.c_double), C.c_double, P(C.c_double),
                                              P(C.c_double), C.c_int64]),
        "deftri_solve_lm": (C.c_int, [C.c_void_p, P(_abi.LMParams), P(_abi.Report)]),
        "deftri_set_lm_lanes": (C.c_int, [C.c_void_p, C.c_int32]),
        "deftri_set_jacobian_mode": (C.c_int, [C.c_void_p, C.c_int32]),
        "deftri_set_factor_precision": (C.c_int, [C.c_void_p, C.c_int32]),
        "deftri_set_linear_solver": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_int32]),
        "deftri_last_step_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "deftri_set_plan": (C.c_int, [C.c_void_p, C.c_int32]),
        "deftri_set_pair_window": (C.c_int, [C.c_void_p, C.c_int32]),
        "deftri_set_jacobian_storage": (C.c_int, [C.c_void_p, C.c_int32]),
        "deftri_get_plan_info": (C.c_int, [C.c_void_p, P(_abi.PlanInfo)]),
        "deftri_debug_sp_product": (C.c_int, [C.c_void_p, P(_abi.ProblemDesc), P(C.c_double), P(C.c_double),
                                              P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_double),
                                              C.c_double, P(C.c_double), P(C.c_double), C.c_int64, P(C.c_int64)]),
        "deftri_pixels_stand_dev": (C.c_int, [C.c_void_p, P(_abi.MapC), P(_abi.PixelsError)]),
        "deftri_triangulate_nrslam": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float),
                                                P(C.c_float), P(C.c_float), P(C.c_float), C.c_float, P(C.c_float),
                                                P(C.c_float), P(C.c_uint8)]),
        "deftri_triangulate": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_float),
                                         P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), C.c_float, P(C.c_float),
                                         P(C.c_float), P(C.c_uint8)]),
        "deftri_reconstruct_points": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float),
                                                P(C.c_float), P(C.c_float), P(C.c_float), P(_abi.ReconstructParams),
                                                P(C.c_float), P(C.c_float), P(C.c_uint8), P(C.c_float),
                                                P(_abi.ReconstructReport)]),
        "deftri_init_depth_scales": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, P(C.c_float), P(C.c_float),
                                               P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float),
                                               P(C.c_float), C.c_float, P(C.c_uint8), P(C.c_double), P(C.c_double),
                                               P(C.c_int64)]),
        "deftri_match_for_initialization": (C.c_int, [C.c_void_p, P(_abi.FeatureGrid), C.c_int32, P(C.c_float), P(C.c_int32),
                                                      P(C.c_uint8), C.c_int32, P(C.c_float), P(C.c_int32), P(C.c_uint8),
                                                      C.c_int32, C.c_float, P(C.c_int32), P(C.c_int32), P(C.c_int32),
                                                      P(C.c_int32)]),
        "deftri_epipolar_inliers": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float),
                                              P(C.c_float), P(C.c_float), C.c_float, P(C.c_uint8), P(C.c_float),
                                              P(C.c_int32)]),
        "deftri_find_essential_ransac": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float),
                                                   C.c_int32, P(C.c_int32), C.c_float, P(C.c_float), P(C.c_uint8), P(C.c_float),
                                                   P(C.c_int32), P(C.c_float), P(C.c_uint8), P(_abi.EssentialReport)]),
        "deftri_reconstruct_cameras": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float),
                                                 P(C.c_uint8), P(C.c_float), P(C.c_float), P(C.c_int32)]),
        "deftri_debug_feature_grid_cells": (C.c_int, [C.c_void_p, P(_abi.FeatureGrid), C.c_int32, P(C.c_float), P(C.c_int32),
                                                      P(C.c_int32)]),
        "deftri_undistort_points": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float), C.c_int32,
                                              P(C.c_float)]),
        "deftri_image_bounds": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, P(C.c_float), P(C.c_float), C.c_int32, P(C.c_float)]),
        "deftri_distribute_features": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32,
                                                 P(C.c_float), P(C.c_float), C.c_int32, C.c_int32, P(C.c_float), P(C.c_float),
                                                 P(_abi.FeatureGrid), P(C.c_int32), P(C.c_int32), P(C.c_uint8)]),
        "deftri_delaunay2d": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_double), C.c_int32, P(C.c_int32), P(_abi.DelaunayReport)]),
        "deftri_set_mesh_builder": (C.c_int, [C.c_void_p, C.c_int32]),
        "deftri_arap_deform": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_double), C.c_int32, P(C.c_int32), C.c_int32, P(C.c_int32),
                                         C.c_int32, P(C.c_double), P(_abi.ArapDeformParams), P(C.c_double), P(C.c_double),
                                         P(_abi.ArapDeformReport)]),
        "deftri_arap_open3d_optimization": (C.c_int, [C.c_void_p, P(_abi.MapC), P(_abi.ArapDeformReport)]),
        "deftri_set_plan_builder": (C.c_int, [C.c_void_p, C.c_int32]),
        "deftri_set_tile_builder": (C.c_int, [C.c_void_p, C.c_int32]),
        "deftri_set_layout_builder": (C.c_int, [C.c_void_p, C.c_int32]),
        "deftri_set_multi_pair_builder": (C.c_int, [C.c_void_p, C.c_int32]),
        "deftri_set_multi_tile_builder": (C.c_int, [C.c_void_p, C.c_int32]),
        "deftri_debug_plan_tile_digest": (C.c_int, [C.c_void_p, P(_abi.ProblemDesc), C.c_int32, C.c_int32, P(C.c_uint64), C.c_int32, P(C.c_int32)]),
        "deftri_debug_plan_layout_stats": (C.c_int, [C.c_void_p, P(_abi.ProblemDesc), C.c_int32, C.c_int32, P(C.c_int64), C.c_int32]),
        "deftri_plan_build_info": (C.c_int, [C.c_void_p, P(C.c_int32), P(C.c_int32), P(C.c_int32), P(C.c_double)]),
        "deftri_set_graph_builder": (C.c_int, [C.c_void_p, C.c_int32]),
        "deftri_graph_build_info": (C.c_int, [C.c_void_p, P(C.c_int32), P(C.c_int32), P(C.c_int32), P(C.c_double)]),
        "deftri_debug_plan_digest": (C.c_int, [C.c_void_p, P(_abi.ProblemDesc), C.c_int32, C.c_int32, P(C.c_uint64), C.c_int32,
                                               P(C.c_int32)]),
        "deftri_debug_delaunay_still_valid": (C.c_int, [C.c_int32, P(C.c_double), C.c_int32, P(C.c_int32)]),
        "deftri_debug_delaunay_sweep": (C.c_int, [C.c_int32, P(C.c_double), C.c_int32, P(C.c_int32), P(C.c_int32), P(C.c_int32)]),
        "deftri_search_with_projection": (C.c_int, [C.c_void_p, P(_abi.FeatureGrid), P(C.c_float), P(C.c_float), C.c_int32,
                                                    P(C.c_float), P(C.c_int32), P(C.c_uint8), P(C.c_int32), C.c_int32,
                                                    P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_uint8),
                                                    C.c_int32, P(C.c_int32), P(C.c_uint8), P(C.c_float), P(C.c_float),
                                                    P(C.c_int32), P(C.c_int32), P(C.c_int32), P(_abi.ProjectionReport)]),
        "deftri_guided_matching": (C.c_int, [C.c_void_p, P(_abi.FeatureGrid), P(C.c_float), P(C.c_float), C.c_int32,
                                             P(C.c_float), P(C.c_int32), P(C.c_uint8), P(C.c_int32), C.c_int32, P(C.c_uint8),
                                             P(C.c_float), P(C.c_int32), P(C.c_uint8), C.c_int32, C.c_int32, P(C.c_int32),
                                             P(C.c_uint8), P(C.c_float), P(C.c_int32), P(C.c_int32), P(_abi.ProjectionReport)]),
        "deftri_map_point_descriptors": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), P(C.c_int32), P(C.c_int32), P(C.c_int32),
                                                   C.c_int32, P(C.c_float), P(C.c_int32), P(C.c_uint8), P(C.c_int32), C.c_int32,
                                                   C.c_float, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_uint8),
                                                   P(C.c_int32), P(C.c_uint8)]),
        "deftri_search_for_triangulation": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), P(C.c_uint8), P(C.c_uint8), C.c_int32,
                                                      P(C.c_float), P(C.c_uint8), P(C.c_uint8), P(C.c_float), P(C.c_float),
                                                      C.c_int32, C.c_float, C.c_int32, P(C.c_int32), P(C.c_int32), P(C.c_uint8),
                                                      P(C.c_int32), P(_abi.TriangulationMatchReport)]),
        "deftri_fuse_search": (C.c_int, [C.c_void_p, P(_abi.FeatureGrid), P(C.c_float), P(C.c_float), C.c_int32, P(C.c_float),
                                         P(C.c_int32), P(C.c_uint8), C.c_int32, P(C.c_uint8), P(C.c_float), P(C.c_int32),
                                         P(C.c_uint8), C.c_int32, P(C.c_int32), P(C.c_uint8), P(C.c_float), P(C.c_int32),
                                         P(C.c_int32), P(_abi.ProjectionReport)]),
        "deftri_fast_extract": (C.c_int, [C.c_void_p, P(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, P(C.c_uint8), C.c_int32,
                                          C.c_int32, C.c_int32, P(_abi.FastParams), P(C.c_float), P(C.c_int32), P(C.c_float),
                                          P(C.c_float), P(C.c_float), P(C.c_int32), P(_abi.FastReport)]),
        "deftri_debug_fast_pyramid": (C.c_int, [C.c_void_p, P(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, P(_abi.FastParams),
                                                C.c_int32, P(C.c_uint8), P(C.c_int32), P(C.c_int32)]),
        "deftri_debug_fast_candidates": (C.c_int, [C.c_void_p, P(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, P(_abi.FastParams),
                                                   C.c_int32, C.c_int32, P(C.c_int32), P(C.c_float), P(C.c_int32)]),
        "deftri_debug_fast_mask": (C.c_int, [C.c_void_p, P(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, P(C.c_uint8), C.c_int32,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_int32), P(C.c_uint8)]),
        "deftri_orb_set_pattern": (C.c_int, [C.c_void_p, P(C.c_int32)]),
        "deftri_orb_describe": (C.c_int, [C.c_void_p, P(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, P(_abi.OrbParams), C.c_int32,
                                          P(C.c_float), P(C.c_int32), P(C.c_float), P(C.c_uint8), P(C.c_uint8), P(_abi.OrbReport)]),
        "deftri_debug_orb_pyramid": (C.c_int, [C.c_void_p, P(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, P(_abi.OrbParams),
                                               C.c_int32, P(C.c_uint8), P(C.c_int32), P(C.c_int32)]),
        "deftri_debug_orb_blur_kernel": (C.c_int, [P(C.c_int32)]),
        "deftri_download": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double), P(C.c_double)]),
        "deftri_reset_state": (C.c_int, [C.c_void_p]),
        "deftri_eval_chi2": (C.c_int, [C.c_void_p, P(C.c_double)]),
        "deftri_eval_gradient": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double), C.c_int64]),
        "deftri_eval_hessian_product": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double), C.c_int64]),
        "deftri_eval_damped_solve": (C.c_int, [C.c_void_p, C.c_double, P(C.c_double), P(C.c_double), C.c_int64]),
        "deftri_num_unknowns": (C.c_int64, [C.c_void_p]),
        "deftri_sizeof": (C.c_int64, [C.c_int32]),
        "deftri_profile_trial": (C.c_int, [C.c_void_p, C.c_double, P(_abi.KernelStat), C.c_int32, P(C.c_int32)]),
        "deftri_arap_graph_point_ids": (C.c_int, [C.c_void_p, P(C.c_int64), C.c_int64]),
        "deftri_graph_stats": (C.c_int, [C.c_void_p, P(C.c_int64), P(C.c_int64), P(C.c_double)]),
        "deftri_graph_repairs": (C.c_int, [C.c_void_p, P(C.c_int64), P(C.c_int64)]),
        "deftri_arap_build_graph": (C.c_int, [C.c_void_p, P(_abi.MapC), C.c_double, C.c_double, C.c_float,
                                              P(P(_abi.ProblemDesc))]),
        "deftri_arap_optimization": (C.c_int, [C.c_void_p, P(_abi.MapC), C.c_double, C.c_double, C.c_double,
                                               C.c_double, C.c_double, C.c_float, C.c_int32, P(C.c_double),
                                               P(_abi.Report)]),
        "deftri_deformation_optimization": (C.c_int, [C.c_void_p, P(_abi.MapC), P(_abi.DeformationParams),
                                                      P(_abi.DeformationReport)]),
        "deftri_global_insert": (C.c_int, [P(C.c_double), P(C.c_double), P(C.c_double)]),
        "deftri_keyframe_order": (C.c_int, [P(C.c_int64), C.c_int32, C.c_int32, P(C.c_int64)]),
        "deftri_debug_nelder_mead": (C.c_int, [_abi.OBJECTIVE_FN, C.c_void_p, C.c_int32, P(C.c_double), P(C.c_double),
                                               P(C.c_double), C.c_double, C.c_double, C.c_int32, P(C.c_double),
                                               P(C.c_int32), P(C.c_int32)]),
        # bundle adjustment
        "deftri_ba_create": (C.c_int, [C.c_int32, P(C.c_void_p)]),
        "deftri_ba_destroy": (C.c_int, [C.c_void_p]),
        "deftri_ba_last_error": (C.c_char_p, [C.c_void_p]),
        "deftri_ba_upload": (C.c_int, [C.c_void_p, P(_abi.BADesc)]),
        "deftri_ba_set_state": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double)]),
        "deftri_ba_set_edge_flags": (C.c_int, [C.c_void_p, P(C.c_uint8), P(C.c_uint8)]),
        "deftri_ba_solve_lm": (C.c_int, [C.c_void_p, P(_abi.LMParams), C.c_int32, P(_abi.Report)]),
        "deftri_ba_compute_errors": (C.c_int, [C.c_void_p, P(C.c_uint8)]),
        "deftri_ba_edge_chi2": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_uint8)]),
        "deftri_ba_download": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double)]),
        "deftri_ba_eval_system": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, P(C.c_double), P(C.c_double),
                                            P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_int32)]),
        "deftri_rccl_unique_id": (C.c_int, [P(C.c_uint8)]),
        "deftri_dist_init_rccl": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, P(C.c_uint8)]),
        "deftri_dist_set_transport": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _abi.XFER_FN, C.c_void_p]),
        "deftri_dist_vertex_owner": (C.c_int, [C.c_void_p, P(C.c_int32), C.c_int64]),
        "deftri_plan_vertex_order": (C.c_int, [C.c_void_p, P(C.c_int64), C.c_int64]),
        "deftri_measure_sim_absolute_map_errors": (C.c_int, [C.c_int32, P(_abi.MapC), C.c_int32, P(C.c_float),
                                                             P(C.c_float), P(_abi.AbsErrorsC)]),
        "deftri_measure_relative_map_errors": (C.c_int, [C.c_int32, P(_abi.MapC), P(_abi.RelErrorsC), C.c_int32,
                                                         P(C.c_int32)]),
        "deftri_sim_normal_stream": (C.c_int, [C.c_int64, C.c_float, C.c_float, P(C.c_float)]),
        "deftri_set_depth_images": (C.c_int, [C.c_void_p, C.c_int32, P(_abi.DepthImageC)]),
        "deftri_depth_measure": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, P(C.c_float), C.c_int32, P(C.c_double),
                                           P(C.c_uint8)]),
        "deftri_depth_image_stats": (C.c_int, [C.c_void_p, P(C.c_int64), P(C.c_int64)]),
        "deftri_measure_real_absolute_map_errors": (C.c_int, [C.c_void_p, P(_abi.MapC), P(_abi.RealAbsErrorsC)]),
        "deftri_measure_relative_map_errors_images": (C.c_int, [C.c_void_p, P(_abi.MapC), P(_abi.RelErrorsC), C.c_int32,
                                                                P(C.c_int32)]),
        "deftri_sim_two_view": (C.c_int, [C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float),
                                          P(C.c_float), P(C.c_float), C.c_float, C.c_int32, C.c_float, C.c_float,
                                          C.c_float, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float),
                                          P(C.c_float), P(C.c_float)]),
        "deftri_dist_owned_edges": (C.c_int, [C.c_void_p, P(C.c_uint8), P(C.c_uint8), P(C.c_uint8)]),
        "deftri_debug_plan_solve_dist": (C.c_int, [C.c_void_p, P(C.c_double), C.c_double, P(C.c_double),
                                                   P(C.c_double), C.c_int64]),
        "deftri_ba_dist_init_rccl": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, P(C.c_uint8)]),
        "deftri_ba_dist_set_allreduce": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _abi.ALLREDUCE_FN,
                                                   C.c_void_p]),
        "deftri_ba_profile_trial": (C.c_int, [C.c_void_p, C.c_double, P(_abi.KernelStat), C.c_int32,
                                              P(C.c_int32)]),
    }
    dev_build = "DEFTRI_LIB" in os.environ          # an older build under A/B may lack newer entry points
    for name, (res, args) in sig.items():
        if dev_build and not hasattr(lib, name):
            continue
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    _lib = lib
    return lib


EXPORTED = [
    "deftri_abi_version", "deftri_ctx_create", "deftri_ctx_destroy", "deftri_last_error",
    "deftri_problem_upload", "deftri_problem_analyse", "deftri_plan_stats", "deftri_debug_plan_solve",
    "deftri_solve_lm", "deftri_set_lm_lanes", "deftri_set_jacobian_mode", "deftri_set_factor_precision", "deftri_set_linear_solver", "deftri_last_step_info", "deftri_pixels_stand_dev", "deftri_triangulate_nrslam", "deftri_download", "deftri_reset_state", "deftri_eval_chi2",
    "deftri_eval_gradient", "deftri_eval_hessian_product", "deftri_eval_damped_solve",
    "deftri_num_unknowns", "deftri_sizeof", "deftri_arap_build_graph", "deftri_arap_graph_point_ids", "deftri_graph_stats", "deftri_graph_repairs", "deftri_arap_optimization",
    "deftri_profile_trial",
    "deftri_ba_create", "deftri_ba_destroy", "deftri_ba_last_error", "deftri_ba_upload", "deftri_ba_set_state",
    "deftri_ba_set_edge_flags", "deftri_ba_solve_lm", "deftri_ba_compute_errors", "deftri_ba_edge_chi2",
    "deftri_ba_download", "deftri_ba_eval_system", "deftri_rccl_unique_id", "deftri_ba_dist_init_rccl",
    "deftri_ba_dist_set_allreduce", "deftri_ba_profile_trial",
    "deftri_dist_init_rccl", "deftri_dist_set_transport", "deftri_dist_vertex_owner", "deftri_plan_vertex_order", "deftri_sim_two_view", "deftri_sim_normal_stream",
    "deftri_measure_sim_absolute_map_errors", "deftri_measure_relative_map_errors", "deftri_dist_owned_edges",
    "deftri_debug_plan_solve_dist", "deftri_set_plan", "deftri_set_jacobian_storage", "deftri_get_plan_info",
    "deftri_debug_sp_product", "deftri_set_pair_window", "deftri_deformation_optimization", "deftri_global_insert",
    "deftri_debug_nelder_mead", "deftri_keyframe_order",
    "deftri_set_depth_images", "deftri_depth_measure", "deftri_depth_image_stats",
    "deftri_measure_real_absolute_map_errors", "deftri_measure_relative_map_errors_images",
    "deftri_triangulate", "deftri_reconstruct_points", "deftri_init_depth_scales",
    "deftri_match_for_initialization", "deftri_epipolar_inliers", "deftri_debug_feature_grid_cells",
    "deftri_search_with_projection", "deftri_guided_matching", "deftri_map_point_descriptors",
    "deftri_find_essential_ransac", "deftri_reconstruct_cameras",
    "deftri_search_for_triangulation", "deftri_fuse_search",
    "deftri_fast_extract", "deftri_debug_fast_pyramid", "deftri_debug_fast_candidates", "deftri_debug_fast_mask",
    "deftri_orb_set_pattern", "deftri_orb_describe", "deftri_debug_orb_pyramid", "deftri_debug_orb_blur_kernel",
    "deftri_undistort_points", "deftri_image_bounds", "deftri_distribute_features",
    "deftri_delaunay2d", "deftri_set_mesh_builder", "deftri_debug_delaunay_still_valid", "deftri_debug_delaunay_sweep",
    "deftri_set_plan_builder", "deftri_plan_build_info", "deftri_debug_plan_digest", "deftri_set_tile_builder",
    "deftri_set_layout_builder", "deftri_debug_plan_layout_stats", "deftri_set_multi_pair_builder",
    "deftri_set_graph_builder", "deftri_graph_build_info", "deftri_set_multi_tile_builder", "deftri_debug_plan_tile_digest",
    "deftri_arap_deform", "deftri_arap_open3d_optimization",
]

# the digests of deftri_debug_plan_tile_digest, in its order
PLAN_TILE_DIGEST_NAMES = ("tile_trow", "tile_tdst", "tile_poff", "tile_nshare", "tile_scalars", "combined")

# the figures of deftri_debug_plan_layout_stats, in its order
PLAN_LAYOUT_STATS = ("waves", "split_waves", "two_window_waves", "zero_step_waves", "slot_steps", "blocks", "depth_blocks",
                     "max_heavy_run")

# the arrays of deftri_debug_plan_digest, in its order; the combined digest follows them
PLAN_DIGEST_NAMES = (
    "row_of_point", "point_of_row", "rank_row_begin", "arap_ids", "rep_ids", "dep_ids", "rot_ids", "arap_rot_local",
    "blk", "hv_blk", "hv_blk_off", "dperm", "inc_off", "inc", "rep_off", "dep_off", "rowmap", "woff", "wsplit", "pmap",
    "pidx", "tile_tab", "tile_m0", "tile_m1", "tile_chunk", "tile_rs", "tile_halo", "tile_xoff", "tile_xdst",
    "send_rows", "recv_rows", "scalars", "combined")


def trian_method_code(method):
    """Triangulation.method as useTriangulationMethod's `if` chain reads it (Geometry.cc:220-228): any
    string other than the three named ones is NRSLAM."""
    return {"Classic": _abi.DEFTRI_TRI_CLASSIC, "ORBSLAM": _abi.DEFTRI_TRI_ORBSLAM,
            "DepthMeasurement": _abi.DEFTRI_TRI_DEPTH}.get(method, _abi.DEFTRI_TRI_NRSLAM)


def trian_location_code(location):
    """Triangulation.seed.location as the triangulate* functions read it: any string other than
    "TwoPoints" / "FarPoints" is the in-rays seed."""
    return {"TwoPoints": _abi.DEFTRI_LOC_TWOPOINTS, "FarPoints": _abi.DEFTRI_LOC_FARPOINTS}.get(location, _abi.DEFTRI_LOC_INRAYS)


def _pose34(T):
    """Sophus::SE3f::matrix3x4() of an SE3f (R, t): float32 [3, 4]."""
    return np.ascontiguousarray(np.concatenate([np.asarray(T.R, np.float32), np.asarray(T.t, np.float32)[:, None]], 1),
                                np.float32)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _image_u8(a, what="image"):
    """An 8-bit single-channel image as (array with contiguous rows, rows, cols, row stride in bytes); a row
    stride wider than the row (a view of a wider image) is passed on as it is."""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError(f"{what}: an 8-bit single-channel image (uint8 [rows, cols]) is required, got {a.dtype} {a.shape}")
    if a.shape[1] > 0 and (a.strides[1] != 1 or a.strides[0] < a.shape[1]):
        a = np.ascontiguousarray(a)
    return a, a.shape[0], a.shape[1], (a.strides[0] if a.shape[0] > 1 else a.shape[1])


class FastResult:
    """The keypoints of Context.fast_extract, in the reference's order: uv float32 [n, 2], octave int32 [n],
    angle (degrees), response and size float32 [n], and the report (deftri_fast_report as a dict)."""

    def __init__(self, uv, octave, angle, response, size, report):
        self.uv, self.octave, self.angle, self.response, self.size, self.report = uv, octave, angle, response, size, report

    def __len__(self):
        return len(self.octave)


class OrbResult:
    """The descriptors of Context.orb_describe: desc uint8 [n, 32], status uint8 [n] (1: a sample outside the
    bordered level, the descriptor is zero), and the report (deftri_orb_report as a dict)."""

    def __init__(self, desc, status, report):
        self.desc, self.status, self.report = desc, status, report

    def __len__(self):
        return len(self.status)


class DistributedFeatures:
    """The result of Context.distribute_features: uv float32 [n, 2] the undistorted keys (Frame::vKeys_), grid (the
    dict of deftri_feature_grid's fields every matcher takes), cell_start int32 [cols * rows + 1] and cell_items int32
    [n] (grid_[col][row] as a CSR over cells col * rows + row, keypoint order within a cell, -1 behind the last
    list), in_grid bool [n]."""

    def __init__(self, uv, grid, cell_start, cell_items, in_grid):
        self.uv, self.grid, self.cell_start, self.cell_items, self.in_grid = uv, grid, cell_start, cell_items, in_grid

    def __len__(self):
        return len(self.uv)

    def cells(self):
        """grid_[col][row] as nested lists, the shape matching.build_grid returns."""
        cols, rows = self.grid["cols"], self.grid["rows"]
        s = self.cell_start
        return [[self.cell_items[s[c * rows + r]:s[c * rows + r + 1]].tolist() for r in range(rows)] for c in range(cols)]


class ProjectionMatchResult:
    """The result of Context.search_with_projection / .guided_matching: match int32 [n] (the frame's slot or -1),
    status uint8 [n] (0 matched, 1 view cosine, 2 distance, 3 no candidates, 4 rejected, 5 undefined in the
    reference, 6 reference slot without a map point), uv float32 [n, 2] the projections, best / second int32 [n],
    slot_point int32 [n2] the frame's slots after the call, report (deftri_projection_report as a dict), and for
    search_with_projection view_cos float32 [n] and predicted_octave int32 [n]."""

    def __init__(self, match, status, uv, best, second, slot_point, report, view_cos=None, predicted_octave=None):
        self.match, self.status, self.uv, self.best, self.second = match, status, uv, best, second
        self.slot_point, self.report, self.view_cos, self.predicted_octave = slot_point, report, view_cos, predicted_octave


class TriangulationMatchResult:
    """The result of Context.search_for_triangulation: matches int32 [n1] (the keypoint of keyframe 2 or -1), best_dist
    int32 [n1] (255 where the row was never accepted), status uint8 [n1] (0 matched, 1 slot occupied, 2 no eligible
    candidate below th, 3 matched and then robbed by a later row, 4 passed over by the flag quirk), n_matches (the
    reference's return value) and report (deftri_triangulation_match_report as a dict)."""

    def __init__(self, matches, best_dist, status, n_matches, report):
        self.matches, self.best_dist, self.status, self.n_matches, self.report = matches, best_dist, status, n_matches, report


class EssentialResult:
    """The result of Context.find_essential_ransac: E float32 [3, 3] the best model (zero when there is none),
    inlier bool [n] and err float32 [n] under it (NaN without one), scores int32 [n_hyp], E_all float32 [n_hyp, 3, 3],
    degenerate bool [n_hyp], report (deftri_essential_report as a dict; report["best"] is -1 when every score is 0)."""

    def __init__(self, E, inlier, err, scores, E_all, degenerate, report):
        self.E, self.inlier, self.err, self.scores, self.E_all, self.degenerate, self.report = E, inlier, err, scores, E_all, degenerate, report


class MapPointDescriptors:
    """The result of Context.map_point_descriptors: normal float32 [n, 3], max_dist / min_dist float32 [n], desc
    uint8 [n, 32], ref_obs int32 [n] (the chosen observation's ordinal), status uint8 [n] (1: no observation,
    nothing written for the point)."""

    def __init__(self, normal, max_dist, min_dist, desc, ref_obs, status):
        self.normal, self.max_dist, self.min_dist, self.desc, self.ref_obs, self.status = normal, max_dist, min_dist, desc, ref_obs, status


def _i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _pixel_pairs(uv1, uv2):
    """Two matched pixel lists as float32 [n, 2] each, and n."""
    uv1, uv2 = _f32(uv1).reshape(-1, 2), _f32(uv2).reshape(-1, 2)
    assert len(uv2) == len(uv1)
    return uv1, uv2, len(uv1)


class Context:
    """One solver context (one per host thread).  device < 0 = host-only (graph / analysis)."""

    def __init__(self, device=0):
        self.h = None                    # close() / __del__ after a failed create
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.deftri_ctx_create(int(device), C.byref(h))
        if rc != 0:
            raise DeftriError(rc, "deftri_ctx_create failed (no usable gfx950 device?)" if device >= 0 else "ctx")
        self.h = h
        self.device = device
        self._desc = None
        self._prob = None
        self._solver = ("pcg", 0.0, 0)
        self.jacobian_mode = False       # deftri_set_jacobian_mode's default: g2o numeric Jacobians
        self._images_sig = ()            # the depth image set on the context (register_depth_images)
        self._images_digest = ()

    def set_jacobian_mode(self, analytic):
        """The Jacobians of deftri_arap_optimization / _deformation_optimization on this context."""
        self._check(self.lib.deftri_set_jacobian_mode(self.h, 1 if analytic else 0))
        self.jacobian_mode = bool(analytic)

    def close(self):
        if getattr(self, "h", None):
            self.lib.deftri_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise DeftriError(rc, (self.lib.deftri_last_error(self.h) or b"").decode())

    # flat-graph API ------------------------------------------------------------------------
    def upload(self, prob: Problem):
        self._prob = prob
        self._desc = prob.to_desc()
        self._check(self.lib.deftri_problem_upload(self.h, C.byref(self._desc)))

    def analyse(self, prob: Problem):
        self._prob = prob
        self._desc = prob.to_desc()
        self._check(self.lib.deftri_problem_analyse(self.h, C.byref(self._desc)))

    def plan_stats(self):
        r = _abi.Report()
        self._check(self.lib.deftri_plan_stats(self.h, C.byref(r)))
        return {k: v for k, v in r.as_dict().items() if k in ("n_unknowns", "nnz_factor", "factor_flops", "n_fronts", "n_levels")}

    def debug_plan_solve(self, H, lam, rhs):
        H = np.ascontiguousarray(H, dtype=np.float64)
        r = np.ascontiguousarray(rhs, dtype=np.float64)
        x = np.zeros_like(r)
        self._check(self.lib.deftri_debug_plan_solve(self.h, _dp(H), float(lam), _dp(r), _dp(x), len(r)))
        return x

    # point-sharded solve ---------------------------------------------------------------------
    def dist_init_rccl(self, nranks, rank, uid):
        """RCCL communicator (uid: 128 bytes from rccl_unique_id() on rank 0)."""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(uid))
        self._check(self.lib.deftri_dist_init_rccl(self.h, int(nranks), int(rank), buf))

    def dist_set_transport(self, nranks, rank, transport):
        """Host-memory transport: `transport(op, peer, array)` with op 0 sum / 1 max all-reduce in
        place, 2 send, 3 receive (array: float64 view of the staging buffer); returns 0."""
        def cb(_user, op, peer, buf, n):
            try:
                arr = np.ctypeslib.as_array(buf, shape=(int(n),)) if n > 0 else np.zeros(0)
                return int(transport(int(op), int(peer), arr) or 0)
            except Exception as e:           # never let an exception cross the C frames
                import sys
                print(f"deftri transport callback failed: {e!r}", file=sys.stderr, flush=True)
                return -1
        self._xfer_cb = _abi.XFER_FN(cb) if nranks > 1 else _abi.XFER_FN()
        self._check(self.lib.deftri_dist_set_transport(self.h, int(nranks), int(rank), self._xfer_cb, None))

    def vertex_owner(self):
        nv = self._prob.n_pairs + self._prob.n_scales + self._prob.n_points
        out = np.zeros(nv, np.int32)
        self._check(self.lib.deftri_dist_vertex_owner(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), nv))
        return out

    def vertex_order(self):
        nv = self._prob.n_pairs + self._prob.n_scales + self._prob.n_points
        out = np.zeros(nv, np.int64)
        self._check(self.lib.deftri_plan_vertex_order(self.h, out.ctypes.data_as(C.POINTER(C.c_int64)), nv))
        return out

    def owned_edges(self):
        p = self._prob
        r, d, a = (np.zeros(max(k, 1), np.uint8) for k in (len(p.rep_point), len(p.dep_point), len(p.arap_pair)))
        u8 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint8))
        self._check(self.lib.deftri_dist_owned_edges(self.h, u8(r), u8(d), u8(a)))
        return (r[:len(p.rep_point)].astype(bool), d[:len(p.dep_point)].astype(bool), a[:len(p.arap_pair)].astype(bool))

    def debug_plan_solve_dist(self, Hq, lam, bq):
        Hq = np.ascontiguousarray(Hq, dtype=np.float64)
        bq = np.ascontiguousarray(bq, dtype=np.float64)
        x = np.zeros_like(bq)
        self._check(self.lib.deftri_debug_plan_solve_dist(self.h, _dp(Hq), float(lam), _dp(bq), _dp(x), len(bq)))
        return x

    def set_linear_solver(self, solver="pcg", tol=0.0, max_iterations=0):
        """LM step solver: "pcg" (block-Jacobi PCG, LDL^T fallback; default) or "direct" (multifrontal LDL^T)."""
        code = {"direct": _abi.DEFTRI_SOLVER_DIRECT, "pcg": _abi.DEFTRI_SOLVER_PCG}[solver]
        self._check(self.lib.deftri_set_linear_solver(self.h, code, float(tol), int(max_iterations)))
        self._solver = (solver, tol, max_iterations)

    def set_plan(self, plan="auto"):
        """Plan kind of the next upload: "auto", "multifrontal" (LDL^T analysis; sliced matrix-free PCG
        where it fits) or "iterative" (point-sharded matrix-free PCG, no factorization; csrc/spcg.h)."""
        code = {"auto": _abi.DEFTRI_PLAN_AUTO, "multifrontal": _abi.DEFTRI_PLAN_MULTIFRONTAL,
                "iterative": _abi.DEFTRI_PLAN_ITERATIVE}[plan]
        self._check(self.lib.deftri_set_plan(self.h, code))

    def set_pair_window(self, window):
        """Graph builds: 0 every keyframe pair (the reference), w > 0 pairs at most w apart in map order."""
        self._check(self.lib.deftri_set_pair_window(self.h, int(window)))

    def set_jacobian_storage(self, fp32):
        """Iterative plan: the ARAP Jacobians the product reads in fp32 (1) or fp64 (0, default)."""
        self._check(self.lib.deftri_set_jacobian_storage(self.h, 1 if fp32 else 0))

    def plan_info(self):
        info = _abi.PlanInfo()
        self._check(self.lib.deftri_get_plan_info(self.h, C.byref(info)))
        return info.as_dict()

    def debug_sp_product(self, prob, jarap, warap, jrep, wrep, jdep, wdep, lam, p):
        """Host emulation of the iterative plan's product on this rank (deftri_debug_sp_product):
        returns (q with this rank's rows + the global vertices, [own rows, halo rows, local ARAP
        edges, owned ARAP edges])."""
        d = prob.to_desc()
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        arrs = [f(a) for a in (jarap, warap, jrep, wrep, jdep, wdep, p)]
        q = np.zeros(prob.n_unknowns)
        st = np.zeros(4, np.int64)
        self._check(self.lib.deftri_debug_sp_product(self.h, C.byref(d), *[_dp(a) for a in arrs[:6]], float(lam),
                                                     _dp(arrs[6]), _dp(q), prob.n_unknowns,
                                                     st.ctypes.data_as(C.POINTER(C.c_int64))))
        return q, st

    def last_step_info(self):
        """(CG iterations, converged) of the last PCG step."""
        it, ok = C.c_int32(), C.c_int32()
        self._check(self.lib.deftri_last_step_info(self.h, C.byref(it), C.byref(ok)))
        return it.value, bool(ok.value)

    def set_factor_precision(self, fp32_updates):
        """1: trailing updates on fp32 MFMA (the C5 precision sweep); 0: fp64 (default, the reference's)."""
        self._check(self.lib.deftri_set_factor_precision(self.h, 1 if fp32_updates else 0))

    def set_lm_lanes(self, lanes):
        """Speculative lambda lanes (0 = default, 1 = sequential trials); results are identical."""
        self._check(self.lib.deftri_set_lm_lanes(self.h, int(lanes)))

    def solve_lm(self, n_iterations=10, analytic=False, tau=1e-5, max_trials=10, user_lambda=0.0, verbose=False):
        prm = _abi.LMParams(n_iterations=n_iterations, max_trials=max_trials, tau=tau, user_lambda=user_lambda,
                            analytic_jacobians=1 if analytic else 0, verbose=1 if verbose else 0)
        rep = _abi.Report()
        self._check(self.lib.deftri_solve_lm(self.h, C.byref(prm), C.byref(rep)))
        return rep.as_dict()

    def download(self):
        p = self._prob
        pts = np.zeros((p.n_points, 3)); sc = np.zeros(p.n_scales); tg = np.zeros((p.n_pairs, 7))
        self._check(self.lib.deftri_download(self.h, _dp(pts), _dp(sc), _dp(tg)))
        return pts, sc, tg

    def reset_state(self):
        self._check(self.lib.deftri_reset_state(self.h))

    def chi2(self):
        v = C.c_double()
        self._check(self.lib.deftri_eval_chi2(self.h, C.byref(v)))
        return v.value

    def gradient(self):
        n = self._prob.n_unknowns
        b = np.zeros(n); d = np.zeros(n)
        self._check(self.lib.deftri_eval_gradient(self.h, _dp(b), _dp(d), n))
        return b, d

    def hessian_product(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        self._check(self.lib.deftri_eval_hessian_product(self.h, _dp(x), _dp(y), len(x)))
        return y

    def damped_solve(self, lam, rhs, solver="direct", tol=0.0, max_iterations=0):
        """(H + lam I) x = rhs with `solver` ("direct" LDL^T or "pcg"); the context's solver setting
        is restored afterwards."""
        r = np.ascontiguousarray(rhs, dtype=np.float64)
        x = np.zeros_like(r)
        prev = self._solver
        self.set_linear_solver(solver, tol, max_iterations)
        try:
            self._check(self.lib.deftri_eval_damped_solve(self.h, float(lam), _dp(r), _dp(x), len(r)))
        finally:
            self.set_linear_solver(*prev)
        return x

    def profile_trial(self, lam):
        """Per-kernel device time of one LM trial: {name: {launches, ms, flops, bytes}}."""
        arr = (_abi.KernelStat * 64)()
        n = C.c_int32()
        self._check(self.lib.deftri_profile_trial(self.h, float(lam), arr, 64, C.byref(n)))
        return {arr[i].name.decode(): {"launches": arr[i].launches, "ms": arr[i].ms, "flops": arr[i].flops,
                                       "bytes": arr[i].bytes} for i in range(n.value)}

    # keyframe depth images -------------------------------------------------------------------
    def set_depth_images(self, images):
        """deftri_set_depth_images: `images` = [(kf id, float32 [rows, cols], image_depth_scale, ph[4])];
        replaces the context's set ([] clears it)."""
        arr = (_abi.DepthImageC * max(1, len(images)))()
        keep = []
        for n, (kid, im, scale, ph) in enumerate(images):
            im = np.ascontiguousarray(im, np.float32)
            keep.append(im)
            arr[n].kf_id, arr[n].rows, arr[n].cols = int(kid), im.shape[0], im.shape[1]
            arr[n].pixels = _abi.ptr(im, _abi.f32)
            arr[n].image_depth_scale = float(scale)
            arr[n].ph[:] = [float(v) for v in ph]
        self._images_sig = self._images_digest = None      # unknown until register_depth_images sets them
        self._check(self.lib.deftri_set_depth_images(self.h, len(images), arr))

    def register_depth_images(self, m):
        """The depth images of a Map's keyframes on the context, before a map-level call: sent only
        when the set changed (the same arrays, or other arrays with the same content — the clones a
        worker process receives)."""
        images = getattr(m, "depth_images", None)                # sim.ArrayMap (simulated scenes) carries none
        kfs = sorted(images() if images else [], key=lambda kf: kf.id)   # a clone iterates its keyframes in another order
        sig =tuple((kf.id, kf.depth_image.ctypes.data, kf.depth_image.shape, float(kf.image_depth_scale),
                     tuple(float(v) for v in kf.ph)) for kf in kfs)
        if sig == self._images_sig:
            return
        import zlib
        digest = tuple((s[0], zlib.crc32(kf.depth_image), zlib.adler32(kf.depth_image)) + s[2:] for s, kf in zip(sig, kfs))
        if digest != self._images_digest:
            self.set_depth_images([(kf.id, kf.depth_image, kf.image_depth_scale, kf.ph) for kf in kfs])
        self._images_sig, self._images_digest = sig, digest
        self._images_keep = [kf.depth_image for kf in kfs]      # the addresses in `sig` stay theirs

    def depth_measure(self, kf_id, uv, scaled=True):
        """KeyFrame::getDepthMeasure(x, y, scaled) of keyframe kf_id's image for the pixels uv [n, 2]:
        (depth [n] float64, NaN where the status is not 0; status [n] uint8 — deftri.h)."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        n = len(uv)
        depth = np.zeros(n, np.float64); status = np.zeros(n, np.uint8)
        self._check(self.lib.deftri_depth_measure(self.h, int(kf_id), n, _abi.ptr(uv, _abi.f32), 1 if scaled else 0,
                                                  _dp(depth), _abi.ptr(status, C.c_uint8)))
        return depth, status

    def depth_image_stats(self):
        """(images copied to the context, keyframe samplings) over the context's life."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.deftri_depth_image_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def measure_real_absolute(self, m):
        """deftri_measure_real_absolute_map_errors (Measurements.cc:101-348); figures in mm."""
        self.register_depth_images(m)
        mc, keep = m.to_c()
        out = _abi.RealAbsErrorsC()
        self._check(self.lib.deftri_measure_real_absolute_map_errors(self.h, C.byref(mc), C.byref(out)))
        return {k: getattr(out, k) for k, _ in _abi.RealAbsErrorsC._fields_}

    def measure_relative_images(self, m):
        """deftri_measure_relative_map_errors_images: one record per keyframe pair."""
        self.register_depth_images(m)
        mc, keep = m.to_c()
        K = len(m.keyframes)
        npair = max(1, K * (K - 1) // 2)
        out = (_abi.RelErrorsC * npair)()
        n = C.c_int32()
        self._check(self.lib.deftri_measure_relative_map_errors_images(self.h, C.byref(mc), out, npair, C.byref(n)))
        return [{k: getattr(out[i], k) for k, _ in _abi.RelErrorsC._fields_} for i in range(n.value)]

    # map-level API -------------------------------------------------------------------------
    def build_graph(self, m, rep_weight, arap_weight, depth_error):
        self.register_depth_images(m)
        mc, keep = m.to_c()
        out = C.POINTER(_abi.ProblemDesc)()
        self._check(self.lib.deftri_arap_build_graph(self.h, C.byref(mc), float(rep_weight), float(arap_weight),
                                                     C.c_float(depth_error), C.byref(out)))
        p = Problem.from_desc(out.contents)
        ids = np.zeros(p.n_points, np.int64)
        self._check(self.lib.deftri_arap_graph_point_ids(self.h, ids.ctypes.data_as(C.POINTER(C.c_int64)), p.n_points))
        p.point_ids = ids
        return p

    def set_mesh_builder(self, mode):
        """Who triangulates a keyframe in the graph builds of this context (deftri_set_mesh_builder): 0 the host
        sweep (the default), 1 the star path of Context.delaunay.  The graph is the same bit for bit."""
        self._check(self.lib.deftri_set_mesh_builder(self.h, int(mode)))

    def set_graph_builder(self, mode):
        """Who runs the passes of a full graph build of this context (deftri_set_graph_builder): 0 the host (the
        default), 1 the device stages where they apply (a device context, the direct id table, no skipped point).
        The graph is the same array for array; no effect on a host-only context."""
        self._check(self.lib.deftri_set_graph_builder(self.h, int(mode)))

    def graph_build_info(self):
        """What the last full graph build did (deftri_graph_build_info): builder_used, stages (bit mask, 0x3f for a
        device build), reason (0 none, 1 not applicable, 2 an input error, 3 a mesh handed back), ms."""
        used, stages, reason, ms = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
        self._check(self.lib.deftri_graph_build_info(self.h, C.byref(used), C.byref(stages), C.byref(reason), C.byref(ms)))
        return dict(builder_used=used.value, stages=stages.value, reason=reason.value, ms=ms.value)

    def set_plan_builder(self, mode):
        """Who builds the iterative plan at the next upload of this context (deftri_set_plan_builder): 0 the host
        passes (default), 1 the device stages where they apply (one rank, one pair, the tile layout)."""
        self._check(self.lib.deftri_set_plan_builder(self.h, int(mode)))

    def set_tile_builder(self, mode):
        """Who cuts the one-pair tile layout where plan builder 1's device stages apply (deftri_set_tile_builder):
        0 build_tiles on the host (default), 1 the device stages (plan_build_info stages bits 6-9).  No effect with
        plan builder 0."""
        self._check(self.lib.deftri_set_tile_builder(self.h, int(mode)))

    def set_layout_builder(self, mode):
        """Who builds the phase-1 blocks and the phase-2 wave layout where plan builder 1 and tile builder 1 both ran
        (deftri_set_layout_builder): 0 the host (default), 1 the device stages (plan_build_info stages bits 10-12);
        an upload then keeps pmap and pidx on the device.  On several pairs under set_multi_pair_builder(1): the wave
        layout alone (bits 11-12).  No effect anywhere else."""
        self._check(self.lib.deftri_set_layout_builder(self.h, int(mode)))

    def set_multi_pair_builder(self, mode):
        """Whether plan builder 1's device stages also take a problem of several keyframe pairs
        (deftri_set_multi_pair_builder): 0 no (default), 1 yes — one rank, the tile layout requested; plan_build_info
        stages 0x3f, with layout builder 1 0x183f (stage 8b; an upload then keeps pmap and pidx on the device).
        build_tiles_multi (unless set_multi_tile_builder(1)) and stage 7 stay on the host.  No effect with plan builder 0
        or on one pair."""
        self._check(self.lib.deftri_set_multi_pair_builder(self.h, int(mode)))

    def set_multi_tile_builder(self, mode):
        """Who cuts the tile layout of several pairs where set_multi_pair_builder(1)'s device stages apply
        (deftri_set_multi_tile_builder): 0 the host's build_tiles_multi (default), 1 the device stages — plan_build_info
        stages 0x3ff, with layout builder 1 0x1bff.  A graph build_tiles_multi refuses goes to the host after the
        device's rows (0x7).  No effect on one pair or with plan or multi-pair builder 0."""
        self._check(self.lib.deftri_set_multi_tile_builder(self.h, int(mode)))

    def plan_build_info(self):
        """What the last iterative plan build did (deftri_plan_build_info): builder_used, stages (bit mask),
        reason (0 none, 1 not applicable, 2 a bounded loop reached its bound), ms."""
        used, stages, reason, ms = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
        self._check(self.lib.deftri_plan_build_info(self.h, C.byref(used), C.byref(stages), C.byref(reason), C.byref(ms)))
        return dict(builder_used=used.value, stages=stages.value, reason=reason.value, ms=ms.value)

    def debug_plan_digest(self, prob, mode, tile):
        """(names, digests) of the plan an upload would build with builder `mode`, the tile layout requested or
        not (deftri_debug_plan_digest): one FNV-1a digest per plan array, the combined digest last."""
        d = prob.to_desc()
        out = np.zeros(len(PLAN_DIGEST_NAMES), np.uint64)
        n = C.c_int32()
        self._check(self.lib.deftri_debug_plan_digest(self.h, C.byref(d), int(mode), int(tile),
                                                      out.ctypes.data_as(C.POINTER(C.c_uint64)), len(out), C.byref(n)))
        assert n.value == len(PLAN_DIGEST_NAMES), n.value
        return PLAN_DIGEST_NAMES, [int(x) for x in out]

    def debug_plan_tile_digest(self, prob, mode, tile):
        """FNV-1a digests of the arrays and scalars only a multi-pair tile plan holds, of the plan debug_plan_digest
        builds (deftri_debug_plan_tile_digest): (PLAN_TILE_DIGEST_NAMES, digests)."""
        d = prob.to_desc()
        out = np.zeros(len(PLAN_TILE_DIGEST_NAMES), np.uint64)
        n = C.c_int32(0)
        self._check(self.lib.deftri_debug_plan_tile_digest(self.h, C.byref(d), int(mode), int(tile),
                                                           out.ctypes.data_as(C.POINTER(C.c_uint64)), len(out), C.byref(n)))
        assert n.value == len(PLAN_TILE_DIGEST_NAMES), n.value
        return PLAN_TILE_DIGEST_NAMES, [int(x) for x in out]

    def debug_plan_layout_stats(self, prob, mode, tile):
        """Figures of the phase-1 blocks and the wave layout of the plan debug_plan_digest builds
        (deftri_debug_plan_layout_stats), as a dict with the keys PLAN_LAYOUT_STATS."""
        d = prob.to_desc()
        out = np.zeros(len(PLAN_LAYOUT_STATS), np.int64)
        self._check(self.lib.deftri_debug_plan_layout_stats(self.h, C.byref(d), int(mode), int(tile),
                                                            out.ctypes.data_as(C.POINTER(C.c_int64)), len(out)))
        return dict(zip(PLAN_LAYOUT_STATS, (int(x) for x in out)))

    def delaunay(self, xy, tris_cap=None):
        """The Delaunay triangulation of xy [n, 2] (deftri_delaunay2d) on this context: stars on the device, or on
        the host with exact predicates on a host-only one.  Returns (tris int32 [T, 3], counter-clockwise, each
        starting at its smallest vertex, sorted; report dict): the library's host sweep, triangle for triangle.
        All points on a line raise DeftriError (DEFTRI_E_GRAPH)."""
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        n = len(xy)
        cap = 2 * n + 1 if tris_cap is None else int(tris_cap)
        tris = np.zeros((max(cap, 1), 3), np.int32)
        rep = _abi.DelaunayReport()
        self._check(self.lib.deftri_delaunay2d(self.h, n, _dp(xy), cap, tris.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(rep)))
        return tris[:rep.n_tris].copy(), rep.as_dict()

    def arap_deform(self, vertices, tris, constraint_ids, constraint_positions, max_iter=50, energy="spokes",
                    smoothed_alpha=0.01, cg_tol=None, cg_max_iterations=None):
        """As-rigid-as-possible deformation of the mesh (vertices [n, 3], tris [T, 3]) with the handles
        constraint_ids -> constraint_positions (deftri_arap_deform: Open3D's DeformAsRigidAsPossible restated, the
        global step by PCG on this context's device, or in host loops on a host-only context).  energy "spokes" or
        "smoothed".  Returns (positions [n, 3], energies [max_iter], report dict).  A DeftriError raised by the call
        carries the report filled so far as `.report`."""
        v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
        cid = np.ascontiguousarray(constraint_ids, np.int32).reshape(-1)
        cpos = np.ascontiguousarray(constraint_positions, np.float64).reshape(-1, 3)
        codes = {"spokes": 0, "smoothed": 1}
        prm = _abi.ArapDeformParams()
        prm.max_iter = int(max_iter)
        prm.energy = codes[energy.lower()] if isinstance(energy, str) else int(energy)
        prm.smoothed_alpha = float(smoothed_alpha)
        prm.cg_tol = 0.0 if cg_tol is None else float(cg_tol)
        prm.cg_max_iterations = 0 if cg_max_iterations is None else int(cg_max_iterations)
        out = np.zeros_like(v)
        en = np.zeros(max(int(max_iter), 0), np.float64)
        rep = _abi.ArapDeformReport()
        rc = self.lib.deftri_arap_deform(self.h, len(v), _dp(v), len(t), _ip(t), len(cid), _ip(cid), len(cpos), _dp(cpos),
                                         C.byref(prm), _dp(out), _dp(en) if len(en) else None, C.byref(rep))
        try:
            self._check(rc)
        except DeftriError as e:
            e.report = rep.as_dict()
            raise
        return out, en, rep.as_dict()

    def arap_open3d_optimization(self, m):
        """arapOpen3DOptimization(Map*) (g2oBundleAdjustment.cc:1010-1104; deftri_arap_open3d_optimization): every
        keyframe pair's mesh deformed by arap_deform with the reference's arguments, the map's positions written back
        as fp32.  Returns the last pair's report dict.  On an error the map is unchanged."""
        mc, keep = m.to_c()
        rep = _abi.ArapDeformReport()
        t = time.perf_counter()
        rc = self.lib.deftri_arap_open3d_optimization(self.h, C.byref(mc), C.byref(rep))
        self.last_call_s = time.perf_counter() - t
        self._check(rc)
        for kid, _pid, pos, *_rest in keep["arrays"]:      # positions only: this entry moves nothing else (:1079-1082)
            for i, mp in enumerate(m.keyframes[kid].map_points):
                if mp is not None:
                    mp.position = pos[i].copy()
        return rep.as_dict()

    def graph_repairs(self):
        """(keyframe meshes of full graph builds repaired from the previous build's triangulation, their
        flips) over this context's life."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.deftri_graph_repairs(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def graph_stats(self):
        """(memo hits, structure-memo hits, host ms of the last graph build)."""
        a, b, t = C.c_int64(), C.c_int64(), C.c_double()
        self._check(self.lib.deftri_graph_stats(self.h, C.byref(a), C.byref(b), C.byref(t)))
        return a.value, b.value, t.value

    def pixels_stand_dev(self, m):
        """calculatePixelsStandDev (Geometry.cc:370-498) of a Map on the device."""
        mc, keep = m.to_c()
        out = _abi.PixelsError()
        self._check(self.lib.deftri_pixels_stand_dev(self.h, C.byref(mc), C.byref(out)))
        return out.as_dict()

    def triangulate_nrslam(self, uv1, uv2, kb8_1, kb8_2, T1w, T2w, min_cos=0.9998):
        """Mapping::triangulateSimulatedMapPoints (NRSLAM, FarPoints) on the device.  T1w/T2w: SE3f
        (R, t).  Returns (x3d_1 [n,3], x3d_2 [n,3], valid [n] bool), fp32."""
        return self.triangulate(uv1, uv2, kb8_1, kb8_2, T1w, T2w, min_cos, method="NRSLAM", location="FarPoints")

    def triangulate(self, uv1, uv2, kb8_1, kb8_2, T1w, T2w, min_cos=0.9998, method="NRSLAM", location="FarPoints"):
        """triangulate_nrslam for any (Triangulation.method, Triangulation.seed.location) the reference
        defines (deftri_triangulate); the strings map as the reference's `if` chains do.  "ORBSLAM" and
        "DepthMeasurement" raise DeftriError (DEFTRI_E_ARG): undefined in the reference (deftri.h)."""
        uv1, uv2, n = _pixel_pairs(uv1, uv2)
        Ta, Tb, k1, k2 = _pose34(T1w), _pose34(T2w), _f32(kb8_1), _f32(kb8_2)
        x1 = np.zeros((n, 3), np.float32); x2 = np.zeros((n, 3), np.float32); v = np.zeros(n, np.uint8)
        self._check(self.lib.deftri_triangulate(self.h, n, trian_method_code(method), trian_location_code(location), _fp(uv1),
                                                _fp(uv2), _fp(k1), _fp(k2), _fp(Ta), _fp(Tb), float(min_cos), _fp(x1), _fp(x2),
                                                _u8p(v)))
        return x1, x2, v.astype(bool)

    def reconstruct_points(self, uv1, uv2, kb8_1, kb8_2, T1w, T2w, method="NRSLAM", location="FarPoints", depth_limit=0.0,
                           checks=False, min_parallax=0.0):
        """MonocularMapInitializer::reconstructPoints for matched pixel pairs on the device
        (deftri_reconstruct_points).  Returns (x3d_1 [n,3], x3d_2 [n,3], status [n] uint8, cos_parallax
        [n] float32, report dict)."""
        uv1, uv2, n = _pixel_pairs(uv1, uv2)
        Ta, Tb, k1, k2 = _pose34(T1w), _pose34(T2w), _f32(kb8_1), _f32(kb8_2)
        prm = _abi.ReconstructParams(method=trian_method_code(method), location=trian_location_code(location),
                                     checks=1 if checks else 0, depth_limit=float(depth_limit),
                                     min_parallax=float(min_parallax))
        rep = _abi.ReconstructReport()
        x1 = np.zeros((n, 3), np.float32); x2 = np.zeros((n, 3), np.float32)
        st = np.zeros(n, np.uint8); cosp = np.zeros(n, np.float32)
        self._check(self.lib.deftri_reconstruct_points(self.h, n, _fp(uv1), _fp(uv2), _fp(k1), _fp(k2), _fp(Ta), _fp(Tb),
                                                       C.byref(prm), _fp(x1), _fp(x2), _u8p(st), _fp(cosp), C.byref(rep)))
        return x1, x2, st, cosp, rep.as_dict()

    def init_depth_scales(self, kf_id_1, kf_id_2, uv1, uv2, x3d_1, x3d_2, kb8_1, kb8_2, T1w, T2w, min_cos=0.9998,
                          out=None):
        """The initial estimatedDepthScale_ of two keyframes whose depth images are on the context
        (deftri_init_depth_scales, Mapping.cc:183-254).  Returns (keep [n] bool, scale_1, scale_2,
        n_points); the scales are NaN when n_points == 0.  `out`: a (keep uint8 [n], scales float64 [2],
        n_points int64 [1]) triple to write into instead of new arrays."""
        uv1, uv2, n = _pixel_pairs(uv1, uv2)
        x1, x2 = _f32(x3d_1).reshape(-1, 3), _f32(x3d_2).reshape(-1, 3)
        assert len(x1) == n and len(x2) == n
        Ta, Tb, k1, k2 = _pose34(T1w), _pose34(T2w), _f32(kb8_1), _f32(kb8_2)
        keep, sc, npts = out if out is not None else (np.zeros(n, np.uint8), np.zeros(2, np.float64), np.zeros(1, np.int64))
        s1 = C.cast(sc.ctypes.data, C.POINTER(C.c_double))
        s2 = C.cast(sc.ctypes.data + 8, C.POINTER(C.c_double))
        self._check(self.lib.deftri_init_depth_scales(self.h, int(kf_id_1), int(kf_id_2), n, _fp(uv1), _fp(uv2), _fp(x1), _fp(x2),
                                                      _fp(k1), _fp(k2), _fp(Ta), _fp(Tb), float(min_cos), _u8p(keep), s1, s2,
                                                      npts.ctypes.data_as(C.POINTER(C.c_int64))))
        return keep.astype(bool), float(sc[0]), float(sc[1]), int(npts[0])

    @staticmethod
    def _feature_grid(grid):
        """A deftri_feature_grid from an _abi.FeatureGrid or a dict of its fields (matching.feature_grid)."""
        return grid if isinstance(grid, _abi.FeatureGrid) else _abi.FeatureGrid(**grid)

    def match_for_initialization(self, grid, uv1, octave1, desc1, uv2, octave2, desc2, th, window_size_factor):
        """searchForInitializaion (DescriptorMatching.cc:39-99) of reference keypoints 1 against current
        keypoints 2 on this context: the device, or the sequential host loop on a host-only one
        (deftri_match_for_initialization).  desc: uint8 [n, 32].  Returns (matches int32 [n1] with -1 for
        none, best_dist int32 [n1], second_dist int32 [n1], n_matches)."""
        f = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1, 2)
        uv1, uv2 = f(uv1), f(uv2)
        o1, o2 = np.ascontiguousarray(octave1, np.int32).ravel(), np.ascontiguousarray(octave2, np.int32).ravel()
        d1, d2 = (np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in (desc1, desc2))
        n1, n2 = len(uv1), len(uv2)
        assert len(o1) == n1 and len(d1) == n1 and len(o2) == n2 and len(d2) == n2
        g = self._feature_grid(grid)
        matches = np.zeros(n1, np.int32); best = np.zeros(n1, np.int32); second = np.zeros(n1, np.int32)
        nm = C.c_int32(0)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        bp = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        self._check(self.lib.deftri_match_for_initialization(self.h, C.byref(g), n1, fp(uv1), ip(o1), bp(d1), n2, fp(uv2),
                                                             ip(o2), bp(d2), int(th), float(window_size_factor), ip(matches),
                                                             ip(best), ip(second), C.byref(nm)))
        return matches, best, second, int(nm.value)

    def epipolar_inliers(self, uv1, uv2, kb8_1, kb8_2, T1w, T2w, epipolar_th):
        """The inlier mask of MonocularMapInitializer::initialize with Triangulation.checks for matched
        pixel pairs (deftri_epipolar_inliers).  Returns (inlier bool [n], err float32 [n], score)."""
        uv1, uv2, n = _pixel_pairs(uv1, uv2)
        Ta, Tb, k1, k2 = _pose34(T1w), _pose34(T2w), _f32(kb8_1), _f32(kb8_2)
        inl = np.zeros(n, np.uint8); err = np.zeros(n, np.float32)
        score = C.c_int32(0)
        self._check(self.lib.deftri_epipolar_inliers(self.h, n, _fp(uv1), _fp(uv2), _fp(k1), _fp(k2), _fp(Ta), _fp(Tb),
                                                     float(epipolar_th), _u8p(inl), _fp(err), C.byref(score)))
        return inl.astype(bool), err, int(score.value)

    def find_essential_ransac(self, uv1, uv2, kb8_1, kb8_2, samples, epipolar_th):
        """findEssentialWithRANSAC (MonocularMapInitializer.cc:119-178) with a model per hypothesis for matched pixel
        pairs (deftri_find_essential_ransac): samples int [n_hyp, 8] the match indices each hypothesis is fitted to.
        Every hypothesis is scored against every match on the device, or in sequential loops on a host-only
        context.  Returns an EssentialResult."""
        uv1, uv2, n = _pixel_pairs(uv1, uv2)
        k1, k2 = _f32(kb8_1).reshape(8), _f32(kb8_2).reshape(8)
        smp = np.ascontiguousarray(samples, np.int32)
        if smp.ndim != 2 or smp.shape[1] != 8:
            raise ValueError(f"find_essential_ransac: samples must be [n_hyp, 8], got {smp.shape}")
        H = len(smp)
        E = np.zeros((3, 3), np.float32); inl = np.zeros(n, np.uint8); err = np.zeros(n, np.float32)
        scores = np.zeros(H, np.int32); E_all = np.zeros((H, 3, 3), np.float32); deg = np.zeros(H, np.uint8)
        rep = _abi.EssentialReport()
        self._check(self.lib.deftri_find_essential_ransac(self.h, n, _fp(uv1), _fp(uv2), _fp(k1), _fp(k2), H, _ip(smp),
                                                          float(epipolar_th), _fp(E), _u8p(inl), _fp(err), _ip(scores), _fp(E_all),
                                                          _u8p(deg), C.byref(rep)))
        return EssentialResult(E, inl.astype(bool), err, scores, E_all, deg.astype(bool), rep.as_dict())

    def reconstruct_cameras(self, uv1, uv2, kb8_1, kb8_2, E, use=None):
        """reconstructCameras (MonocularMapInitializer.cc:246-262) for matched pixel pairs (deftri_reconstruct_cameras):
        E float [3, 3], use bool [n] the matches that vote (None: all).  Returns (T2w as an SE3f (Rgood, t), away)."""
        from .mapmodel import SE3f
        uv1, uv2, n = _pixel_pairs(uv1, uv2)
        k1, k2 = _f32(kb8_1).reshape(8), _f32(kb8_2).reshape(8)
        E = _f32(E).reshape(3, 3)
        T = np.zeros((3, 4), np.float32)
        away = C.c_int32(0)
        u = None
        if use is not None:
            u = np.ascontiguousarray(use, np.uint8).reshape(-1)
            if len(u) != n:
                raise ValueError(f"reconstruct_cameras: {n} matches and {len(u)} flags")
        self._check(self.lib.deftri_reconstruct_cameras(self.h, n, _fp(uv1), _fp(uv2), _fp(k1), _fp(k2),
                                                        None if u is None else _u8p(u), _fp(E), _fp(T), C.byref(away)))
        return SE3f(T[:, :3].copy(), T[:, 3].copy()), int(away.value)

    def _frame_arrays(self, Tcw, kb8, uv2, octave2, desc2):
        """The current frame's arguments of the projection matchers."""
        T = _pose34(Tcw) if hasattr(Tcw, "R") else _f32(Tcw).reshape(3, 4)
        uv2 = _f32(uv2).reshape(-1, 2); o2 = _i32(octave2)
        d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        if not (len(uv2) == len(o2) == len(d2)):
            raise ValueError(f"{len(uv2)} keypoints, {len(o2)} octaves and {len(d2)} descriptors")
        return T, _f32(kb8).reshape(8), uv2, o2, d2

    def search_with_projection(self, grid, Tcw, kb8, uv2, octave2, desc2, slot_point, pos, normal, min_dist, max_dist, desc, th):
        """searchWithProjection (DescriptorMatching.cc:164-253) on this context: the device, or the sequential
        host loop on a host-only one (deftri_search_with_projection).  Tcw: an SE3f or float [3, 4]; slot_point
        int [n2]: -1 free, -2 occupied (not modified; the result carries the slots after the call).  Returns a
        ProjectionMatchResult."""
        T, k, uv2, o2, d2 = self._frame_arrays(Tcw, kb8, uv2, octave2, desc2)
        slot = _i32(slot_point).copy()
        pos = _f32(pos).reshape(-1, 3); nrm = _f32(normal).reshape(-1, 3)
        mn, mx = _f32(min_dist).reshape(-1), _f32(max_dist).reshape(-1)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n, n2 = len(pos), len(uv2)
        if not (len(nrm) == len(mn) == len(mx) == len(d) == n) or len(slot) != n2:
            raise ValueError("search_with_projection: array lengths differ")
        g = self._feature_grid(grid)
        match = np.full(n, -1, np.int32); status = np.zeros(n, np.uint8); uv = np.zeros((n, 2), np.float32)
        vc = np.zeros(n, np.float32); po = np.full(n, -1, np.int32)
        best = np.full(n, 255, np.int32); second = np.full(n, 255, np.int32)
        rep = _abi.ProjectionReport()
        self._check(self.lib.deftri_search_with_projection(self.h, C.byref(g), _fp(T), _fp(k), n2, _fp(uv2), _ip(o2), _u8p(d2),
                                                           _ip(slot), n, _fp(pos), _fp(nrm), _fp(mn), _fp(mx), _u8p(d), int(th),
                                                           _ip(match), _u8p(status), _fp(uv), _fp(vc), _ip(po), _ip(best),
                                                           _ip(second), C.byref(rep)))
        return ProjectionMatchResult(match, status, uv, best, second, slot, rep.as_dict(), vc, po)

    def guided_matching(self, grid, Tcw, kb8, uv2, octave2, desc2, has_point, pos, octave1, desc, th, window_size_factor):
        """guidedMatching (DescriptorMatching.cc:101-162) on this context (deftri_guided_matching).  Per reference
        slot: has_point bool [n1], and where it is set pos [n1, 3], octave1 [n1], desc uint8 [n1, 32] of the slot's
        map point.  Returns a ProjectionMatchResult whose slot_point holds reference slots."""
        T, k, uv2, o2, d2 = self._frame_arrays(Tcw, kb8, uv2, octave2, desc2)
        has = np.ascontiguousarray(has_point, np.uint8).reshape(-1)
        pos = _f32(pos).reshape(-1, 3); o1 = _i32(octave1)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n1, n2 = len(has), len(uv2)
        if not (len(pos) == len(o1) == len(d) == n1):
            raise ValueError("guided_matching: array lengths differ")
        if int(window_size_factor) != window_size_factor:
            raise ValueError("guided_matching: windowSizeFactor is an int in the reference")
        g = self._feature_grid(grid)
        slot = np.full(n2, -1, np.int32)
        match = np.full(n1, -1, np.int32); status = np.where(has != 0, 0, 6).astype(np.uint8); uv = np.zeros((n1, 2), np.float32)
        best = np.full(n1, 255, np.int32); second = np.full(n1, 255, np.int32)
        rep = _abi.ProjectionReport()
        self._check(self.lib.deftri_guided_matching(self.h, C.byref(g), _fp(T), _fp(k), n2, _fp(uv2), _ip(o2), _u8p(d2), _ip(slot),
                                                    n1, _u8p(has), _fp(pos), _ip(o1), _u8p(d), int(th), int(window_size_factor),
                                                    _ip(match), _u8p(status), _fp(uv), _ip(best), _ip(second), C.byref(rep)))
        return ProjectionMatchResult(match, status, uv, best, second, slot, rep.as_dict())

    def search_for_triangulation(self, uv1, desc1, has_point1, uv2, desc2, has_point2, kb8, E, th, epipolar_th, flag_quirk=True):
        """searchForTriangulation (DescriptorMatching.cc:255-328) on this context (deftri_search_for_triangulation): the
        ray and candidate kernels plus the loop over the candidate lists on the device, the loop over all pairs on a
        host-only one.  has_point1 / has_point2 bool [n]: the slot already holds a map point.  flag_quirk: keep the
        reference's vbMatched2[2] (deftri.h).  Returns a TriangulationMatchResult."""
        uv1, uv2 = _f32(uv1).reshape(-1, 2), _f32(uv2).reshape(-1, 2)
        d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32); d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        h1 = np.ascontiguousarray(has_point1, np.uint8).reshape(-1); h2 = np.ascontiguousarray(has_point2, np.uint8).reshape(-1)
        n1, n2 = len(uv1), len(uv2)
        if not (len(d1) == len(h1) == n1 and len(d2) == len(h2) == n2):
            raise ValueError("search_for_triangulation: array lengths differ")
        k = _f32(kb8).reshape(8); E = _f32(E).reshape(3, 3)
        matches = np.full(n1, -1, np.int32); best = np.full(n1, 255, np.int32); status = np.zeros(n1, np.uint8)
        n_matches = C.c_int32(0)
        rep = _abi.TriangulationMatchReport()
        self._check(self.lib.deftri_search_for_triangulation(self.h, n1, _fp(uv1), _u8p(d1), _u8p(h1), n2, _fp(uv2), _u8p(d2),
                                                             _u8p(h2), _fp(k), _fp(E), int(th), float(epipolar_th),
                                                             1 if flag_quirk else 0, _ip(matches), _ip(best), _u8p(status),
                                                             C.byref(n_matches), C.byref(rep)))
        return TriangulationMatchResult(matches, best, status, int(n_matches.value), rep.as_dict())

    def fuse_search(self, grid, Tcw, kb8, uv2, octave2, desc2, consider, pos, octave, desc, th):
        """The search of fuse (DescriptorMatching.cc:330-428) for a list of map points against a keyframe on this context
        (deftri_fuse_search).  Per point: consider bool [n], pos [n, 3], octave [n], desc uint8 [n, 32].  Returns a
        ProjectionMatchResult without slot_point: the map edits are the caller's (matching.fuse)."""
        T, k, uv2, o2, d2 = self._frame_arrays(Tcw, kb8, uv2, octave2, desc2)
        con = np.ascontiguousarray(consider, np.uint8).reshape(-1)
        pos = _f32(pos).reshape(-1, 3); o1 = _i32(octave)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n, n2 = len(con), len(uv2)
        if not (len(pos) == len(o1) == len(d) == n):
            raise ValueError("fuse_search: array lengths differ")
        g = self._feature_grid(grid)
        match = np.full(n, -1, np.int32); status = np.where(con != 0, 0, 6).astype(np.uint8); uv = np.zeros((n, 2), np.float32)
        best = np.full(n, 255, np.int32); second = np.full(n, 255, np.int32)
        rep = _abi.ProjectionReport()
        self._check(self.lib.deftri_fuse_search(self.h, C.byref(g), _fp(T), _fp(k), n2, _fp(uv2), _ip(o2), _u8p(d2), n, _u8p(con),
                                                _fp(pos), _ip(o1), _u8p(d), int(th), _ip(match), _u8p(status), _fp(uv), _ip(best),
                                                _ip(second), C.byref(rep)))
        return ProjectionMatchResult(match, status, uv, best, second, None, rep.as_dict())

    def map_point_descriptors(self, pos, obs_start, obs_kf, obs_slot, kf_Tcw, kf_slot_start, kf_desc, kf_octave, n_scales,
                              scale_factor):
        """Map::updateOrientationAndDescriptor (Map.cc:270-321) for a batch of map points on this context
        (deftri_map_point_descriptors).  Observations as a CSR (obs_start [n + 1] into obs_kf / obs_slot), in the
        order given; keyframes as kf_Tcw float [n_kf, 3, 4] and their slots concatenated (kf_slot_start [n_kf + 1]
        into kf_desc uint8 [slots, 32] and kf_octave [slots]).  Returns a MapPointDescriptors."""
        pos = _f32(pos).reshape(-1, 3)
        os_, ok, osl = _i32(obs_start), _i32(obs_kf), _i32(obs_slot)
        T = _f32(kf_Tcw).reshape(-1, 3, 4); ks = _i32(kf_slot_start)
        kd = np.ascontiguousarray(kf_desc, np.uint8).reshape(-1, 32); ko = _i32(kf_octave)
        n, n_kf = len(pos), len(T)
        if len(os_) != n + 1 or len(ks) != n_kf + 1 or len(ok) != len(osl) or len(kd) != len(ko):
            raise ValueError("map_point_descriptors: array lengths differ")
        if len(ok) != os_[-1] or len(kd) != ks[-1]:
            raise ValueError("map_point_descriptors: the CSR ends do not match the array lengths")
        normal = np.zeros((n, 3), np.float32); mx = np.zeros(n, np.float32); mn = np.zeros(n, np.float32)
        desc = np.zeros((n, 32), np.uint8); ref = np.full(n, -1, np.int32); status = np.zeros(n, np.uint8)
        self._check(self.lib.deftri_map_point_descriptors(self.h, n, _fp(pos), _ip(os_), _ip(ok), _ip(osl), n_kf, _fp(T), _ip(ks),
                                                          _u8p(kd), _ip(ko), int(n_scales), float(scale_factor), _fp(normal),
                                                          _fp(mx), _fp(mn), _u8p(desc), _ip(ref), _u8p(status)))
        return MapPointDescriptors(normal, mx, mn, desc, ref, status)

    def debug_feature_grid_cells(self, grid, uv):
        """TEST ONLY: the cell lists of keypoints `uv` as the match builds them (deftri_debug_feature_grid_cells).
        Returns (cell_start int32 [cols*rows + 1], cell_keys int32 [keys in the grid])."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        g = self._feature_grid(grid)
        start = np.zeros(max(g.cols * g.rows, 0) + 1, np.int32); keys = np.zeros(len(uv), np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self.lib.deftri_debug_feature_grid_cells(self.h, C.byref(g), len(uv), uv.ctypes.data_as(C.POINTER(C.c_float)),
                                                             ip(start), ip(keys)))
        return start, keys[:start[-1]]

    @staticmethod
    def _camera(calib, dist):
        """(calib float32 [4] or None, dist float32 [n_dist], n_dist) of fx, fy, cx, cy and Settings.distortion."""
        dist = _f32(dist if dist is not None else []).reshape(-1)
        calib = None if calib is None else _f32(calib).reshape(-1)
        if calib is not None and len(calib) != 4:
            raise ValueError(f"calib: fx, fy, cx, cy expected, got {len(calib)} values")
        return calib, dist, len(dist)

    def undistort_points(self, uv, calib, dist, in_place=False):
        """cv::undistortPoints(uv, uv, K, dist, Mat(), K) as Frame::undistortKeys calls it (deftri_undistort_points):
        uv float32 [n, 2], calib = fx, fy, cx, cy, dist = k1, k2, p1, p2[, k3].  Returns float32 [n, 2]; with
        in_place the library reads and writes one buffer, as the reference does."""
        uv = np.array(uv, np.float32).reshape(-1, 2) if in_place else _f32(uv).reshape(-1, 2)
        calib, dist, n_dist = self._camera(calib, dist)
        out = uv if in_place else np.zeros_like(uv)
        self._check(self.lib.deftri_undistort_points(self.h, len(uv), _fp(uv), None if calib is None else _fp(calib), _fp(dist),
                                                     n_dist, _fp(out)))
        return out

    def image_bounds(self, cols, rows, calib=None, dist=None):
        """Frame::computeImageBoundaries (deftri_image_bounds): float32 [4] = min_col, min_row, max_col, max_row; no
        distortion coefficients give 0, 0, cols, rows."""
        calib, dist, n_dist = self._camera(calib, dist)
        b = np.zeros(4, np.float32)
        self._check(self.lib.deftri_image_bounds(self.h, int(cols), int(rows), None if calib is None else _fp(calib), _fp(dist),
                                                 n_dist, _fp(b)))
        return b

    def distribute_features(self, grid_cols, grid_rows, n_scales, scale_factor, cols, rows, calib, dist, uv_dis):
        """Frame's bounds and Frame::distributeFeatures for the keypoint slots uv_dis float32 [n, 2]
        (deftri_distribute_features) on this context: the device, or the sequential host loops on a host-only one.
        Returns a DistributedFeatures."""
        uv_dis = _f32(uv_dis).reshape(-1, 2)
        calib, dist, n_dist = self._camera(calib, dist)
        n, ncell = len(uv_dis), max(int(grid_cols), 0) * max(int(grid_rows), 0)
        uv = np.zeros_like(uv_dis); g = _abi.FeatureGrid()
        start = np.zeros((ncell if ncell <= 1 << 24 else 0) + 1, np.int32); items = np.zeros(n, np.int32)
        in_grid = np.zeros(n, np.uint8)
        self._check(self.lib.deftri_distribute_features(self.h, int(grid_cols), int(grid_rows), int(n_scales), float(scale_factor),
                                                        int(cols), int(rows), None if calib is None else _fp(calib), _fp(dist),
                                                        n_dist, n, _fp(uv_dis), _fp(uv), C.byref(g), _ip(start), _ip(items),
                                                        _u8p(in_grid)))
        grid = {k: getattr(g, k) for k, _ in _abi.FeatureGrid._fields_}
        return DistributedFeatures(uv, grid, start, items, in_grid.astype(bool))

    @staticmethod
    def _fast_params(params):
        """A deftri_fast_params from an _abi.FastParams or a dict of its fields (features.fast_params)."""
        return params if isinstance(params, _abi.FastParams) else _abi.FastParams(**params)

    def fast_extract(self, image, params, border_mask=None):
        """FAST::extract (FAST.cc:81-118) of an 8-bit single-channel image on this context: the device, or the
        sequential host loops on a host-only one (deftri_fast_extract).  params: features.fast_params(settings)
        or a dict of deftri_fast_params' fields; border_mask: the decoded FeatureExtractor.imageBoderMask
        (uint8, the image's size) or None.  Returns a FastResult."""
        img, rows, cols, stride = _image_u8(image)
        bm, brows, bcols, bstride = _image_u8(border_mask, "border_mask") if border_mask is not None else (None, 0, 0, 0)
        p = self._fast_params(params)
        cap = max(int(p.max_keys), 0)
        uv = np.zeros((cap, 2), np.float32); octave = np.zeros(cap, np.int32)
        angle = np.zeros(cap, np.float32); response = np.zeros(cap, np.float32); size = np.zeros(cap, np.float32)
        n = C.c_int32(0)
        rep = _abi.FastReport()
        self._check(self.lib.deftri_fast_extract(self.h, _u8p(img), rows, cols, stride, _u8p(bm) if bm is not None else None, brows,
                                                 bcols, bstride, C.byref(p), _fp(uv), octave.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 _fp(angle), _fp(response), _fp(size), C.byref(n), C.byref(rep)))
        k = int(n.value)
        return FastResult(uv[:k], octave[:k], angle[:k], response[:k], size[:k], rep.as_dict())

    def debug_fast_pyramid(self, image, params, level):
        """TEST ONLY: one pyramid level's pixels, uint8 [level rows, level cols] (deftri_debug_fast_pyramid)."""
        img, rows, cols, stride = _image_u8(image)
        p = self._fast_params(params)
        out = np.zeros(max(rows * cols, 1), np.uint8)
        r, c = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.deftri_debug_fast_pyramid(self.h, _u8p(img), rows, cols, stride, C.byref(p), int(level), _u8p(out),
                                                       C.byref(r), C.byref(c)))
        return out[:r.value * c.value].reshape(r.value, c.value).copy()

    def debug_fast_candidates(self, image, params, level):
        """TEST ONLY: one level's candidates in front of distributeOctTree, in the reference's order
        (deftri_debug_fast_candidates).  Returns (xy int32 [n, 2] relative to the 16-pixel border, response
        float32 [n])."""
        img, rows, cols, stride = _image_u8(image)
        p = self._fast_params(params)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        n = C.c_int32(0)
        cap = 0
        while True:
            xy = np.zeros((max(cap, 1), 2), np.int32); resp = np.zeros(max(cap, 1), np.float32)
            self._check(self.lib.deftri_debug_fast_candidates(self.h, _u8p(img), rows, cols, stride, C.byref(p), int(level), cap,
                                                              ip(xy), _fp(resp), C.byref(n)))
            if n.value <= cap:
                return xy[:n.value], resp[:n.value]
            cap = n.value

    def debug_fast_mask(self, image, level, xy, border_mask=None):
        """TEST ONLY: level `level`'s dilated reflection / border mask read at positions xy (x, y) of the image, by
        the method fast_extract uses (deftri_debug_fast_mask).  Returns bool [n]."""
        img, rows, cols, stride = _image_u8(image)
        bm, brows, bcols, bstride = _image_u8(border_mask, "border_mask") if border_mask is not None else (None, 0, 0, 0)
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        hit = np.zeros(max(len(xy), 1), np.uint8)
        self._check(self.lib.deftri_debug_fast_mask(self.h, _u8p(img), rows, cols, stride, _u8p(bm) if bm is not None else None,
                                                    brows, bcols, bstride, int(level), len(xy),
                                                    xy.ctypes.data_as(C.POINTER(C.c_int32)), _u8p(hit)))
        return hit[:len(xy)].astype(bool)

    @staticmethod
    def _orb_params(params):
        """A deftri_orb_params from an _abi.OrbParams or a dict of its fields (features.orb_params)."""
        return params if isinstance(params, _abi.OrbParams) else _abi.OrbParams(**params)

    def orb_set_pattern(self, pattern):
        """The sampling pattern of ORB::describe for this context (deftri_orb_set_pattern): 512 points as an int
        array of shape (512, 2) or (256, 4) (x0 y0 x1 y1 per comparison), in the order of the reference's
        bit_pattern_31_, coordinates in [-15, 15].  A later call replaces it."""
        a = np.asarray(pattern)
        if a.dtype.kind not in "iu" or a.size != 1024 or a.shape not in ((512, 2), (256, 4)):
            raise ValueError(f"pattern: an int array of shape (512, 2) or (256, 4) is required, got {a.dtype} {a.shape}")
        xy = np.ascontiguousarray(a.reshape(-1), np.int32)
        self._check(self.lib.deftri_orb_set_pattern(self.h, xy.ctypes.data_as(C.POINTER(C.c_int32))))

    def orb_describe(self, image, params, uv, octave, angle):
        """ORB::describe (ORB.cc:20-90) of the keypoints (uv [n, 2] full-resolution pixels, octave [n], angle [n]
        in degrees) on an 8-bit single-channel image on this context: the device, or the sequential host loops
        on a host-only one (deftri_orb_describe).  params: features.orb_params(settings) or a dict of
        deftri_orb_params' fields.  Needs orb_set_pattern first.  Returns an OrbResult."""
        img, rows, cols, stride = _image_u8(image)
        p = self._orb_params(params)
        uv = _f32(uv).reshape(-1, 2)
        octave = np.ascontiguousarray(octave, np.int32).reshape(-1)
        angle = _f32(angle).reshape(-1)
        n = len(octave)
        if len(uv) != n or len(angle) != n:
            raise ValueError(f"{len(uv)} keypoints, {n} octaves and {len(angle)} angles")
        desc = np.zeros((n, 32), np.uint8); status = np.zeros(n, np.uint8)
        rep = _abi.OrbReport()
        self._check(self.lib.deftri_orb_describe(self.h, _u8p(img), rows, cols, stride, C.byref(p), n, _fp(uv),
                                                 octave.ctypes.data_as(C.POINTER(C.c_int32)), _fp(angle), _u8p(desc), _u8p(status),
                                                 C.byref(rep)))
        return OrbResult(desc, status, rep.as_dict())

    def debug_orb_pyramid(self, image, params, level):
        """TEST ONLY: one level of orb_describe's pyramid with its 19-pixel border, uint8 [level rows + 38, level
        cols + 38] (deftri_debug_orb_pyramid)."""
        img, rows, cols, stride = _image_u8(image)
        p = self._orb_params(params)
        out = np.zeros((rows + 38) * (cols + 38), np.uint8)
        r, c = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.deftri_debug_orb_pyramid(self.h, _u8p(img), rows, cols, stride, C.byref(p), int(level), _u8p(out),
                                                      C.byref(r), C.byref(c)))
        return out[:r.value * c.value].reshape(r.value, c.value).copy()

    def arap_optimization(self, m, rep_weight, global_weight, arap_weight, alpha, beta, depth_error,
                          n_iterations, want_update=True, analytic=False):
        """analytic=False (default): g2o numeric ARAP/depth Jacobians, the reference's arithmetic."""
        prev = self.jacobian_mode
        self.set_jacobian_mode(analytic)
        self.register_depth_images(m)
        mc, keep = m.to_c()
        upd = C.c_double(0.0)
        rep = _abi.Report()
        t = time.perf_counter()
        try:
            rc = self.lib.deftri_arap_optimization(
                self.h, C.byref(mc), float(rep_weight), float(global_weight), float(arap_weight), float(alpha),
                float(beta), C.c_float(depth_error), int(n_iterations), C.byref(upd) if want_update else None,
                C.byref(rep))
        finally:
            self.set_jacobian_mode(prev)               # the caller's mode again
        self.last_call_s = time.perf_counter() - t     # the C-ABI call alone (no Python marshalling)
        self._check(rc)
        m.from_c(mc, keep)
        return upd.value, rep.as_dict()


    def deformation_optimization(self, m, settings, max_evals=4096):
        """deformationOptimization (g2oBundleAdjustment.cc:446-606) in native code
        (deftri_deformation_optimization): the outer rounds, the Nelder-Mead weight search on map
        clones, arapOptimization and calculatePixelsStandDev on the device.  Writes the map back
        (positions, depth scales, the global table) and returns the report as a dict with the
        evaluation log."""
        settings.validate_for_solver()
        if settings.selection == "open3DArap":
            # optimizationUpdate is never written on this branch and stays 100: every round runs (:481-485)
            n = max(int(settings.n_optimizations), 0)
            t = time.perf_counter()
            for _ in range(n):
                self.arap_open3d_optimization(m)
            return {"rounds": n, "arap_calls": 0, "weights": [float(settings.rep), float(settings.global_), float(settings.arap)],
                    "minf": 0.0, "nlopt_result": 0, "update": 100.0, "seconds": time.perf_counter() - t, "evaluations": [],
                    "round_update": [100.0] * min(n, 64),
                    "round_weights": [[float(settings.rep), float(settings.global_), float(settings.arap)]] * min(n, 64)}
        prm = _abi.DeformationParams()
        # any other selection is the fixed-weight round (:565-568); "twoOptimizations" with a
        # weightsSelection other than "nlopt" too (the Eigen LM returns before evaluating, deftri.h)
        prm.selection = 1 if (settings.selection == "twoOptimizations" and settings.weights_selection == "nlopt") else 0
        prm.rep, prm.global_, prm.arap = float(settings.rep), float(settings.global_), float(settings.arap)
        prm.alpha, prm.beta = float(settings.alpha), float(settings.beta)
        prm.depth_error = float(settings.depth_sigma)
        prm.n_iterations, prm.n_optimizations = int(settings.n_iterations), int(settings.n_optimizations)
        prm.lb[:] = [settings.nlopt_rep_lb, settings.nlopt_global_lb, settings.nlopt_arap_lb]
        prm.ub[:] = [settings.nlopt_rep_ub, settings.nlopt_global_ub, settings.nlopt_arap_ub]
        prm.xtol_rel, prm.xtol_abs = float(settings.nlopt_rel_tol), float(settings.nlopt_abs_tol)
        prm.maxeval = int(settings.nlopt_iterations)
        prm.n_map_points = len(m.map_points)
        evals = (_abi.DeformationEval * max_evals)()
        rep = _abi.DeformationReport()
        rep.evals = C.cast(evals, C.POINTER(_abi.DeformationEval))
        rep.max_evals = max_evals
        self.register_depth_images(m)
        mc, keep = m.to_c()
        prev = self.jacobian_mode
        self.set_jacobian_mode(False)                  # g2o numeric J (the reference's)
        t = time.perf_counter()
        try:
            rc = self.lib.deftri_deformation_optimization(self.h, C.byref(mc), C.byref(prm), C.byref(rep))
        finally:
            self.set_jacobian_mode(prev)               # the caller's mode again
        self.last_call_s = time.perf_counter() - t
        self._check(rc)
        if rep.rounds > 0:
            m.from_c(mc, keep)
        ev = [{"round": evals[k].round, "eval": evals[k].eval, "x": list(evals[k].x), "f": evals[k].f}
              for k in range(min(rep.n_evals, max_evals))]
        return {"rounds": rep.rounds, "arap_calls": rep.arap_calls, "weights": list(rep.weights), "minf": rep.minf,
                "nlopt_result": rep.nlopt_result, "update": rep.update, "seconds": rep.seconds, "evaluations": ev,
                "round_update": list(rep.round_update[:min(rep.rounds, 64)]),
                "round_weights": [list(rep.round_weights[k]) for k in range(min(rep.rounds, 64))]}


def keyframe_order(insert_ids, clones=0):
    """deftri_keyframe_order: the iteration order of Map::mKeyFrames_ (std::unordered_map<ID,
    KeyFrame_>) after inserting `insert_ids` in order, then `clones` Map::clone re-insertions."""
    lib = load()
    n = len(insert_ids)
    a = (C.c_int64 * max(n, 1))(*[int(v) for v in insert_ids])
    out = (C.c_int64 * max(n, 1))()
    rc = lib.deftri_keyframe_order(a, n, int(clones), out)
    if rc:
        raise DeftriError(rc, "deftri_keyframe_order")
    return [int(out[k]) for k in range(n)]


def global_insert(t7):
    """deftri_global_insert: the (0, 1) and (1, 0) entries Map::insertGlobalKeyFramesTransformation
    stores for the solved T_g, as the 7-vectors the next arapOptimization reads (host, no GPU)."""
    lib = load()
    a = (C.c_double * 7)(*[float(v) for v in t7])
    f, i = (C.c_double * 7)(), (C.c_double * 7)()
    rc = lib.deftri_global_insert(a, f, i)
    if rc:
        raise DeftriError(rc, "deftri_global_insert")
    return list(f), list(i)


def nelder_mead_native(f, x0, lb, ub, xtol_rel=0.0, xtol_abs=0.0, maxeval=0):
    """deftri_debug_nelder_mead: the native restated NLopt LN_NELDERMEAD on a Python objective (tests)."""
    lib = load()
    n = len(x0)
    x = (C.c_double * n)(*map(float, x0))
    lo, hi = (C.c_double * n)(*map(float, lb)), (C.c_double * n)(*map(float, ub))
    seen = []

    def cb(xp, nn, user):
        xv = [xp[k] for k in range(nn)]
        seen.append(xv)
        return float(f(xv))
    fn = _abi.OBJECTIVE_FN(cb)
    minf, nev, res = C.c_double(), C.c_int32(), C.c_int32()
    rc = lib.deftri_debug_nelder_mead(fn, None, n, x, lo, hi, float(xtol_rel), float(xtol_abs), int(maxeval),
                                      C.byref(minf), C.byref(nev), C.byref(res))
    if rc:
        raise DeftriError(rc, "deftri_debug_nelder_mead")
    return list(x), minf.value, res.value, nev.value, seen


class BAContext:
    """Bundle-adjustment solver context on one GPU (deftri_ba_*).  `prob` is a ba.BAProblem."""

    def __init__(self, device=0):
        self.h = None                    # close() / __del__ after a failed create
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.deftri_ba_create(int(device), C.byref(h))
        if rc != 0:
            raise DeftriError(rc, "deftri_ba_create failed (no usable gfx950 device?)")
        self.h = h
        self.device = device
        self._prob = None
        self._desc = None
        self._cb = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.deftri_ba_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise DeftriError(rc, (self.lib.deftri_ba_last_error(self.h) or b"").decode())

    def upload(self, prob):
        self._prob = prob
        self._desc = prob.to_desc()
        self._check(self.lib.deftri_ba_upload(self.h, C.byref(self._desc)))

    def set_state(self, poses=None, points=None):
        p = None if poses is None else np.ascontiguousarray(poses, np.float64)
        q = None if points is None else np.ascontiguousarray(points, np.float64)
        self._check(self.lib.deftri_ba_set_state(self.h, None if p is None else _dp(p), None if q is None else _dp(q)))

    def set_edge_flags(self, level=None, robust=None):
        lv = None if level is None else np.ascontiguousarray(level, np.uint8)
        rb = None if robust is None else np.ascontiguousarray(robust, np.uint8)
        self._check(self.lib.deftri_ba_set_edge_flags(self.h, _abi.ptr(lv, C.c_uint8), _abi.ptr(rb, C.c_uint8)))

    def solve_lm(self, n_iterations=10, level=0, tau=1e-5, max_trials=10, user_lambda=0.0, verbose=False):
        prm = _abi.LMParams(n_iterations=n_iterations, max_trials=max_trials, tau=tau, user_lambda=user_lambda,
                            analytic_jacobians=1, verbose=1 if verbose else 0)
        rep = _abi.Report()
        self._check(self.lib.deftri_ba_solve_lm(self.h, C.byref(prm), int(level), C.byref(rep)))
        return rep.as_dict()

    def compute_errors(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self._check(self.lib.deftri_ba_compute_errors(self.h, _abi.ptr(m, C.c_uint8)))

    def edge_chi2(self):
        n = self._prob.n_edges
        chi = np.zeros(n); dp = np.zeros(n, np.uint8)
        self._check(self.lib.deftri_ba_edge_chi2(self.h, _dp(chi), _abi.ptr(dp, C.c_uint8)))
        return chi, dp.astype(bool)

    def download(self):
        p = self._prob
        poses = np.zeros((p.n_poses, 7)); pts = np.zeros((p.n_points, 3))
        self._check(self.lib.deftri_ba_download(self.h, _dp(poses), _dp(pts)))
        return poses, pts

    def eval_system(self, lam, level=0):
        p = self._prob
        K, P = p.n_poses, p.n_points
        ns_max = 6 * K
        S = np.zeros((ns_max, ns_max)); rhs = np.zeros(ns_max)
        dx = np.zeros(6 * K + 3 * P); b = np.zeros(6 * K + 3 * P)
        chi = C.c_double(); ns = C.c_int32()
        self._check(self.lib.deftri_ba_eval_system(self.h, int(level), float(lam), C.byref(chi), _dp(S), _dp(rhs),
                                                   _dp(dx), _dp(b), C.byref(ns)))
        n = ns.value
        S = S.reshape(-1)[:n * n].reshape(n, n).copy()
        return {"chi2": chi.value, "S": S, "rhs": rhs[:n].copy(), "dx": dx, "b": b, "ns": n}

    def dist_init_rccl(self, nranks, rank, uid):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(uid))
        self._check(self.lib.deftri_ba_dist_init_rccl(self.h, int(nranks), int(rank), buf))

    def dist_set_allreduce(self, nranks, rank, fn):
        """fn(np.ndarray view of the host buffer, op) -> None, reducing in place (op 0 sum, 1 max)."""
        def _cb(user, buf, n, op):
            try:
                fn(np.ctypeslib.as_array(buf, shape=(n,)), int(op))
                return 0
            except Exception:                       # noqa: BLE001 — reported as a failed call
                import traceback
                traceback.print_exc()
                return 1
        self._cb = _abi.ALLREDUCE_FN(_cb)
        self._check(self.lib.deftri_ba_dist_set_allreduce(self.h, int(nranks), int(rank), self._cb, None))

    def profile_trial(self, lam):
        arr = (_abi.KernelStat * 64)()
        n = C.c_int32()
        self._check(self.lib.deftri_ba_profile_trial(self.h, float(lam), arr, 64, C.byref(n)))
        return {arr[i].name.decode(): {"launches": arr[i].launches, "ms": arr[i].ms, "flops": arr[i].flops,
                                       "bytes": arr[i].bytes} for i in range(n.value)}


def sim_two_view(orig, moved, c1, c2, kb8_1, kb8_2, rep_error, decimals, depth_error_mm, depth_scales):
    """deftri_sim_two_view: the reference's simulated keypoints / depths / camera poses (SLAM.cc:223-338)."""
    lib = load()
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    orig, moved = f32(orig).reshape(-1, 3), f32(moved).reshape(-1, 3)
    n = len(orig)
    c1, c2, k1, k2 = f32(c1), f32(c2), f32(kb8_1), f32(kb8_2)
    uv1 = np.zeros((n, 2), np.float32); uv2 = np.zeros((n, 2), np.float32)
    d1 = np.zeros(n, np.float32); d2 = np.zeros(n, np.float32)
    p1 = np.zeros(7, np.float32); p2 = np.zeros(7, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = lib.deftri_sim_two_view(n, fp(orig), fp(moved), fp(c1), fp(c2), fp(k1), fp(k2), float(rep_error),
                                 int(decimals), float(depth_error_mm), float(depth_scales[0]),
                                 float(depth_scales[1]), fp(uv1), fp(uv2), fp(d1), fp(d2), fp(p1), fp(p2))
    if rc != 0:
        raise DeftriError(rc, "deftri_sim_two_view")
    return uv1, uv2, d1, d2, p1, p2


def measure_sim_absolute(m, original, moved, device=0):
    """deftri_measure_sim_absolute_map_errors (Measurements.cc:8-98); values in mm."""
    lib = load()
    mc, keep = m.to_c()
    o = np.ascontiguousarray(original, np.float32).reshape(-1, 3)
    mv = np.ascontiguousarray(moved, np.float32).reshape(-1, 3)
    out = _abi.AbsErrorsC()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = lib.deftri_measure_sim_absolute_map_errors(int(device), C.byref(mc), len(o), fp(o), fp(mv), C.byref(out))
    if rc != 0:
        raise DeftriError(rc, "deftri_measure_sim_absolute_map_errors")
    return {k: getattr(out, k) for k, _ in _abi.AbsErrorsC._fields_}


def measure_relative(m, device=0):
    """deftri_measure_relative_map_errors (Measurements.cc:350-518): one record per keyframe pair."""
    lib = load()
    mc, keep = m.to_c()
    K = len(m.keyframes)
    npair = max(1, K * (K - 1) // 2)
    out = (_abi.RelErrorsC * npair)()
    n = C.c_int32()
    rc = lib.deftri_measure_relative_map_errors(int(device), C.byref(mc), out, npair, C.byref(n))
    if rc != 0:
        raise DeftriError(rc, "deftri_measure_relative_map_errors")
    return [{k: getattr(out[i], k) for k, _ in _abi.RelErrorsC._fields_} for i in range(n.value)]


def rccl_unique_id():
    lib = load()
    buf = (C.c_uint8 * 128)()
    rc = lib.deftri_rccl_unique_id(buf)
    if rc != 0:
        raise DeftriError(rc, "ncclGetUniqueId failed")
    return bytes(buf)
