"""ctypes mirror of include/liinit_hip.h.

`Registrar` wraps one `lii_handle`.  Method names follow the reference's vocabulary
(src/laserMapping.cpp, src/IMU_Processing.hpp, include/LI_init/LI_init.h) so that tests read like the
reference's call sites:  map_build ~ ikdtree.Build, map_add_points ~ ikdtree.Add_Points,
undistort_imu/undistort_cv ~ ImuProcess::Process, downsample ~ downSizeFilterSurf.filter,
iekf_update ~ the iterated-Kalman loop of main(), map_incremental ~ map_incremental().
The shared library is mandatory: importing is cheap, but constructing a Registrar raises LIIError when
libliinit_hip.so is missing or no gfx950 device is usable (there is no CPU fallback by design).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (LII_LIB: another build of the same library - A/B measurements of tools/ab.sh; the default is the in-tree build)
_LIB = os.environ.get("LII_LIB") or os.path.join(_HERE, "lib", "libliinit_hip.so")

STATE_DOUBLES = 36 + 576
LII_RADIUS_SORTED = 1  # lii_map_radius flags: every segment ascending in d2


class LIIError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libliinit_hip error {code}: {msg}")
        self.code = code


class lii_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("max_scan_points", C.c_int32),
                ("max_map_points", C.c_int32), ("map_cell_size", C.c_float), ("map_downsample_size", C.c_float),
                ("max_match_dist2", C.c_float), ("reserved0", C.c_float), ("plane_threshold", C.c_double),
                ("laser_point_cov_inv", C.c_double)]


class lii_iekf_opts(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("imu_en", C.c_int32)]


class lii_iekf_report(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("searches", C.c_int32), ("effect_num", C.c_int32),
                ("converged", C.c_int32), ("normal_eq", C.c_double * 91)]


class lii_scan_job(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("undistort", C.c_int32), ("imu_poses", C.c_void_p),
                ("n_imu_poses", C.c_int32), ("leaf", C.c_float), ("opts", lii_iekf_opts), ("scan_dev", C.c_void_p),
                ("n_scan_dev", C.c_int32), ("scan_sorted", C.c_int32), ("map_update", C.c_int32),
                ("next_scan_dev", C.c_void_p), ("next_n_scan", C.c_int32), ("reserved1", C.c_int32),
                ("while_waiting", C.c_void_p), ("while_waiting_arg", C.c_void_p)]


WAIT_HOOK = C.CFUNCTYPE(None, C.c_void_p)  # lii_scan_job::while_waiting


class lii_kernel_profile(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("scans", C.c_int32), ("ms", C.c_double * 8), ("launches", C.c_int32 * 8)]


KERNEL_KINDS = ("deskew", "voxel", "knn", "fit_search", "fit", "solve", "propagate", "publish")  # enum lii_kernel_kind


class lii_publish_opts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("clouds", C.c_int32), ("to_host", C.c_int32), ("save_capacity", C.c_int32)]


class lii_wire_opts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("clouds", C.c_int32), ("to_host", C.c_int32), ("reserved", C.c_int32)]


class lii_wire_field(C.Structure):
    _fields_ = [("name", C.c_char * 16), ("offset", C.c_int32), ("datatype", C.c_int32), ("count", C.c_int32), ("pcd_offset", C.c_int32)]


class lii_wire_layout(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("point_step", C.c_int32), ("n_fields", C.c_int32), ("pcd_row_bytes", C.c_int32),
                ("fields", lii_wire_field * 8)]


class lii_local_map_opts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("enabled", C.c_int32), ("cube_len", C.c_double), ("det_range", C.c_float),
                ("reserved", C.c_int32)]


class lii_local_map_info(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("initialized", C.c_int32), ("cube", C.c_float * 6), ("last_n_boxes", C.c_int32),
                ("last_boxes", C.c_float * 18), ("last_n_deleted", C.c_int32), ("moves", C.c_int32), ("deleted_total", C.c_int64)]


class lii_map_removed_info(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("capacity", C.c_int32), ("held", C.c_int32), ("reserved", C.c_int32),
                ("collected_total", C.c_int64), ("lost_total", C.c_int64)]


class lii_point_noise(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("model", C.c_int32), ("range_inc", C.c_double), ("degree_inc", C.c_double)]


class lii_pose_score(C.Structure):
    _fields_ = [("n_full", C.c_int32), ("effect_num", C.c_int32), ("total_residual", C.c_double)]


POSE_SCORE_DTYPE = np.dtype([("n_full", "<i4"), ("effect_num", "<i4"), ("total_residual", "<f8")])  # struct lii_pose_score as a numpy record
# struct lii_pose_refined as a numpy record (408 bytes)
POSE_REFINED_DTYPE = np.dtype([("pose", "<f8", (12,)), ("cov", "<f8", (6, 6)), ("total_residual", "<f8"), ("effect_num", "<i4"),
                               ("iterations", "<i4"), ("searches", "<i4"), ("flags", "<i4")])
LII_REFINE_CONVERGED, LII_REFINE_BAD_POSE = 1, 2


class lii_surface(C.Structure):  # 88 bytes
    _fields_ = [("count", C.c_int32), ("valid", C.c_int32), ("mean", C.c_double * 3), ("eig", C.c_double * 3), ("normal", C.c_double * 3),
                ("curvature", C.c_double)]


class lii_map_crispness(C.Structure):  # 56 bytes
    _fields_ = [("n_selected", C.c_int64), ("n_used", C.c_int64), ("n_sparse", C.c_int64), ("n_degenerate", C.c_int64), ("mme", C.c_double),
                ("mpv", C.c_double), ("mean_count", C.c_double)]


# struct lii_surface as a numpy record
SURFACE_DTYPE = np.dtype([("count", "<i4"), ("valid", "<i4"), ("mean", "<f8", (3,)), ("eig", "<f8", (3,)), ("normal", "<f8", (3,)), ("curvature", "<f8")])

PUB_DENSE, PUB_DOWN, PUB_EFFECT, PUB_BODY = 1, 2, 4, 8  # lii_publish_opts::clouds
PUB_INTENSITY = 16  # ... the intensities of the DENSE / DOWN / BODY clouds beside them (publish_fetch_intensity)


class lii_imu_sample(C.Structure):
    _fields_ = [("t", C.c_double), ("gyr", C.c_double * 3), ("acc", C.c_double * 3)]


class lii_imu_noise(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32), ("cov_gyr", C.c_double * 3), ("cov_acc", C.c_double * 3),
                ("cov_bias_gyr", C.c_double * 3), ("cov_bias_acc", C.c_double * 3), ("cov_R_LI", C.c_double * 3),
                ("cov_T_LI", C.c_double * 3), ("mean_acc_norm", C.c_double)]


class lii_imu_carry(C.Structure):
    _fields_ = [("last_imu", lii_imu_sample), ("acc_s_last", C.c_double * 3), ("angvel_last", C.c_double * 3),
                ("last_lidar_end_time", C.c_double)]


class lii_pc2_fields(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("point_step", "x", "y", "z", "intensity", "time", "ring")]


class lii_livox_fields(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("point_step", "offset_time", "x", "y", "z", "reflectivity", "tag", "line")]


class lii_ingest_opts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("lidar_type", C.c_int32), ("n_scans", C.c_int32),
                ("point_filter_num", C.c_int32), ("blind", C.c_double), ("stamp_s", C.c_double),
                ("cut_frame_num", C.c_int32), ("scan_count", C.c_int32)]


class lii_frame_info(C.Structure):
    _fields_ = [("begin_time_s", C.c_double), ("last_offset_ms", C.c_double), ("offset", C.c_int32), ("count", C.c_int32)]


class lii_calib_result(C.Structure):
    _fields_ = [("R_LI", C.c_double * 9), ("T_LI", C.c_double * 3), ("gyro_bias", C.c_double * 3),
                ("acc_bias", C.c_double * 3), ("grav_L0", C.c_double * 3), ("time_lag_2", C.c_double),
                ("iterations", C.c_int32 * 3), ("final_cost", C.c_double * 3)]


class lii_li_init_job(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("interpolate", C.c_int32), ("imu", C.c_void_p), ("n_imu", C.c_int32),
                ("lidar", C.c_void_p), ("n_lidar", C.c_int32), ("move_start_time", C.c_double),
                ("orig_odom_freq", C.c_int32), ("cut_frame_num", C.c_int32)]


class lii_li_init_report(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_aligned", C.c_int32), ("n_stage12", C.c_int32), ("n_stage3", C.c_int32),
                ("lag_samples", C.c_int32), ("launches", C.c_int32), ("host_waits", C.c_int32),
                ("termination", C.c_int32 * 3), ("time_lag_1", C.c_double), ("total_time_lag", C.c_double),
                ("params", (C.c_double * 24) * 3)]


class lii_li_init_window(C.Structure):
    _fields_ = [("imu_begin", C.c_int32), ("imu_count", C.c_int32), ("lidar_begin", C.c_int32), ("lidar_count", C.c_int32),
                ("move_start_time", C.c_double)]


class lii_li_init_window_result(C.Structure):
    _fields_ = [("status", C.c_int32), ("pad", C.c_int32), ("res", lii_calib_result), ("rep", lii_li_init_report)]


LII_WIN_OK, LII_WIN_FILTER61, LII_WIN_ALIGNED200, LII_WIN_RAW6, LII_WIN_NO_OVERLAP = 0, 1, 2, 3, 4
# the windows of Registrar.li_init_windows as numpy sees them: lii_li_init_window, field for field
LI_INIT_WINDOW_IN_DTYPE = np.dtype([("imu_begin", "<i4"), ("imu_count", "<i4"), ("lidar_begin", "<i4"), ("lidar_count", "<i4"),
                                    ("move_start_time", "<f8")])
# one record of Registrar.li_init_windows: a window's status (LII_WIN_*), its calibration and what its report says of the run
LI_INIT_WINDOW_DTYPE = np.dtype([("status", "<i4"), ("R_LI", "<f8", (3, 3)), ("T_LI", "<f8", (3,)), ("gyro_bias", "<f8", (3,)),
                                 ("acc_bias", "<f8", (3,)), ("grav_L0", "<f8", (3,)), ("time_lag_1", "<f8"), ("time_lag_2", "<f8"),
                                 ("total_time_lag", "<f8"), ("iterations", "<i4", (3,)), ("final_cost", "<f8", (3,)),
                                 ("termination", "<i4", (3,)), ("n_aligned", "<i4"), ("n_stage12", "<i4"), ("n_stage3", "<i4"),
                                 ("lag_samples", "<i4")])


_DECLS = {
    # name: (restype, argtypes)
    "lii_abi_version": (C.c_int, []),
    "lii_strerror": (C.c_char_p, [C.c_int]),
    "lii_last_error": (C.c_char_p, [C.c_void_p]),
    "lii_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "lii_create": (C.c_int, [C.POINTER(lii_config), C.POINTER(C.c_void_p)]),
    "lii_destroy": (C.c_int, [C.c_void_p]),
    "lii_synchronize": (C.c_int, [C.c_void_p]),
    "lii_map_reset": (C.c_int, [C.c_void_p]),
    "lii_map_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "lii_map_build_xyzi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "lii_map_add_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_map_add_points_xyzi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_map_delete_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_map_delete_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_map_delete_points_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "lii_map_range": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "lii_map_box_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_map_box_search_xyzi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_map_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "lii_map_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_map_download_xyzi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_map_pcd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]),
    "lii_map_intensity_set": (C.c_int, [C.c_void_p, C.c_int32]),
    "lii_map_intensity_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "lii_point_noise_set": (C.c_int, [C.c_void_p, C.POINTER(lii_point_noise)]),
    "lii_point_noise_get": (C.c_int, [C.c_void_p, C.POINTER(lii_point_noise)]),
    "lii_point_noise_download": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32)]),
    "lii_map_commit": (C.c_int, [C.c_void_p]),
    "lii_map_nearest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lii_map_nearest_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lii_map_nearest_xyzi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lii_map_nearest_xyzi_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lii_pose_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "lii_pose_score_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "lii_pose_refine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "lii_pose_refine_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "lii_map_radius": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lii_map_radius_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lii_map_surface": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "lii_map_surface_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "lii_map_crispness": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, C.c_int32, C.POINTER(lii_map_crispness)]),
    "lii_sym3_eigen": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "lii_map_radius_xyzi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lii_map_radius_xyzi_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lii_scan_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "lii_scan_upload_next": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "lii_scan_advance": (C.c_int, [C.c_void_p]),
    "lii_scan_set_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "lii_scan_sort": (C.c_int, [C.c_void_p]),
    "lii_undistort_imu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 4),
    "lii_undistort_cv": (C.c_int, [C.c_void_p] + [C.c_void_p] * 3),
    "lii_downsample": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lii_downsample_skip": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "lii_scan_download": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_ingest_pcl2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(lii_pc2_fields), C.POINTER(lii_ingest_opts),
                                  C.POINTER(lii_frame_info), C.c_int32, C.POINTER(C.c_int32)]),
    "lii_ingest_livox": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(lii_livox_fields), C.POINTER(lii_ingest_opts),
                                   C.POINTER(lii_frame_info), C.c_int32, C.POINTER(C.c_int32)]),
    "lii_frame_select": (C.c_int, [C.c_void_p, C.c_int32]),
    "lii_ingest_pcl2_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(lii_pc2_fields), C.POINTER(lii_ingest_opts)]),
    "lii_ingest_livox_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(lii_livox_fields), C.POINTER(lii_ingest_opts)]),
    "lii_ingest_end": (C.c_int, [C.c_void_p, C.POINTER(lii_frame_info), C.c_int32, C.POINTER(C.c_int32)]),
    "lii_iekf_iterate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lii_iekf_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(lii_iekf_opts),
                                  C.POINTER(lii_iekf_report)]),
    "lii_scan_register": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(lii_iekf_report)]),
    "lii_neighbors_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "lii_last_solve_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "lii_last_unfinished_queries": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "lii_imu_noise_defaults": (C.c_int, [C.POINTER(lii_imu_noise)]),
    "lii_imu_set_noise": (C.c_int, [C.c_void_p, C.POINTER(lii_imu_noise)]),
    "lii_imu_set_carry": (C.c_int, [C.c_void_p, C.POINTER(lii_imu_carry)]),
    "lii_imu_get_carry": (C.c_int, [C.c_void_p, C.POINTER(lii_imu_carry)]),
    "lii_imu_propagate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.POINTER(C.c_int32)]),
    "lii_cv_propagate": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lii_scan_register_imu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                        C.POINTER(lii_iekf_report)]),
    "lii_scan_register_cv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(lii_iekf_report)]),
    "lii_map_build_from_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "lii_local_map_set": (C.c_int, [C.c_void_p, C.POINTER(lii_local_map_opts)]),
    "lii_local_map_get": (C.c_int, [C.c_void_p, C.POINTER(lii_local_map_info)]),
    "lii_local_map_segment": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(lii_local_map_info)]),
    "lii_params_local_map": (C.c_int, [C.c_void_p, C.POINTER(lii_local_map_opts)]),
    "lii_map_removed_set": (C.c_int, [C.c_void_p, C.c_int32]),
    "lii_map_removed_get": (C.c_int, [C.c_void_p, C.POINTER(lii_map_removed_info)]),
    "lii_map_removed_acquire": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "lii_map_removed_acquire_xyzi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "lii_map_removed_view": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "lii_publish_set": (C.c_int, [C.c_void_p, C.POINTER(lii_publish_opts)]),
    "lii_publish_now": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lii_publish_fetch": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "lii_publish_saved": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "lii_publish_fetch_intensity": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "lii_publish_saved_intensity": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_publish_wire_set": (C.c_int, [C.c_void_p, C.POINTER(lii_wire_opts)]),
    "lii_publish_wire_fetch": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "lii_publish_wire_layout": (C.c_int, [C.POINTER(lii_wire_layout)]),
    "lii_publish_saved_pcd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_int32]),
    "lii_pcd_header": (C.c_int, [C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_scan_intensity_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "lii_scan_intensity_set_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "lii_ingest_set_intensity": (C.c_int, [C.c_void_p, C.c_int32]),
    "lii_ingest_set_features": (C.c_int, [C.c_void_p, C.c_int32]),
    "lii_ingest_corners_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_ingest_features_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lii_scan_intensity_download": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_map_incremental": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lii_calib_set_buffers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "lii_calib_eval": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "lii_calib_solve_stage": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(lii_calib_result)]),
    "lii_data_sufficiency": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "lii_li_init_interpolate": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_int32)]),
    "lii_li_init_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                  C.POINTER(lii_calib_result), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "lii_zero_phase_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lii_xcorr_lag": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_li_init_set_device": (C.c_int, [C.c_void_p, C.c_int32]),
    "lii_li_init_resident": (C.c_int, [C.c_void_p, C.POINTER(lii_li_init_job), C.POINTER(lii_calib_result),
                                       C.POINTER(lii_li_init_report)]),
    "lii_li_init_resident_fetch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "lii_calib_solve_stage_dev": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(lii_calib_result)]),
    "lii_li_init_windows": (C.c_int, [C.c_void_p, C.POINTER(lii_li_init_job), C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32]),
    "lii_li_init_windows_scratch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]),
    "lii_comm_unique_id": (C.c_int, [C.c_void_p]),
    "lii_comm_init": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lii_comm_init_ex": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]),
    "lii_comm_describe": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    "lii_comm_transport": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lii_comm_rccl_ranks": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lii_comm_set_partition": (C.c_int, [C.c_void_p, C.c_int32]),
    "lii_comm_destroy": (C.c_int, [C.c_void_p]),
    "lii_selftest_list_exchange": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int32), C.c_int32]),
    "lii_dev_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "lii_dev_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lii_dev_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "lii_params_defaults": (C.c_int, [C.c_void_p]),
    "lii_params_load_yaml": (C.c_int, [C.c_char_p, C.c_void_p]),
    "lii_params_load_launch": (C.c_int, [C.c_char_p, C.c_char_p, C.c_void_p]),
    "lii_params_set": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p]),
    "lii_params_apply": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lii_params_last_error": (C.c_char_p, []),
    "lii_set_profiling": (C.c_int, [C.c_void_p, C.c_int32]),
    "lii_last_timings": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lii_last_kernel_profile": (C.c_int, [C.c_void_p, C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_DECLS)
_lib = None


def library_path() -> str:
    return _LIB


def load_library():
    """dlopen libliinit_hip.so and declare every C-ABI prototype.  Raises LIIError when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            raise LIIError(-2, f"{_LIB} not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no Python/CPU fallback)")
        L = C.CDLL(_LIB)
        for name, (res, args) in _DECLS.items():
            if os.environ.get("LII_LIB") and not hasattr(L, name):
                continue  # (an older build under A/B measurement: what it lacks cannot be called)
            fn = getattr(L, name)  # AttributeError here = the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class _DeviceFloat:
    """... and a buffer of n float32 (the intensity channel)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(int(n),), typestr="<f4", data=(int(ptr), False), version=2)


class _DeviceFloat4:
    """A device buffer the library hands out, as torch reads it (__cuda_array_interface__): n x 4 float32."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(int(n), 4), typestr="<f4", data=(int(ptr), False), version=2)


def _ptr(a):
    # the raw address (ctypes converts an int for a c_void_p parameter); ndarray.ctypes.data_as() is two orders of
    # magnitude slower once a large framework is loaded in the process (measured: 60 us per call next to torch)
    return a.__array_interface__["data"][0]


def wire_layout():
    """lii_publish_wire_layout (host only): dict(point_step, pcd_row_bytes, fields=[(name, offset, datatype, count, pcd_offset), ...]) -
    what fills msg.fields, msg.point_step and msg.row_step of a PointCloud2 made of publish_wire_fetch's bytes."""
    lay = lii_wire_layout(struct_size=C.sizeof(lii_wire_layout))
    rc = load_library().lii_publish_wire_layout(C.byref(lay))
    if rc != 0:
        raise LIIError(rc, "lii_publish_wire_layout")
    return dict(point_step=lay.point_step, pcd_row_bytes=lay.pcd_row_bytes,
                fields=[(f.name.decode(), f.offset, f.datatype, f.count, f.pcd_offset) for f in lay.fields[:lay.n_fields]])


def pcd_header(n_points):
    """lii_pcd_header (host only): the text in front of publish_saved_pcd's rows, as bytes."""
    n = C.c_int32(0)
    buf = C.create_string_buffer(512)
    rc = load_library().lii_pcd_header(int(n_points), buf, len(buf), C.byref(n))
    if rc != 0:
        raise LIIError(rc, "lii_pcd_header")
    return buf.raw[:n.value]


def _dev_address(a):
    """The device address behind `a`: an int, a ctypes pointer, None, or anything with __cuda_array_interface__ (a torch tensor)."""
    if a is None:
        return None
    cai = getattr(a, "__cuda_array_interface__", None)
    if cai is not None:
        return int(cai["data"][0])
    return int(getattr(a, "value", a) or 0) or None


def data_sufficiency(omg, data_accum_length):
    """LI_Init::data_sufficiency_assess (host function of the library): returns (eigenvalues, rot_percent, sufficient)."""
    w = np.ascontiguousarray(omg, np.float64).reshape(-1, 3)
    ev, rp, ok = np.zeros(3), np.zeros(3), C.c_int32(0)
    rc = load_library().lii_data_sufficiency(_ptr(w) if len(w) else None, len(w), float(data_accum_length), _ptr(ev), _ptr(rp), C.byref(ok))
    if rc != 0:
        raise LIIError(rc, "lii_data_sufficiency")
    return ev, rp, bool(ok.value)


def sym3_eigen(m6):
    """lii_sym3_eigen (host function of the library; the device runs the same source): m6 = xx, xy, xz, yy, yz, zz of a symmetric
    3 x 3 matrix.  Returns (eig (3,) ascending, vec (3, 3): row k = the unit eigenvector of eig[k])."""
    m = np.ascontiguousarray(m6, np.float64).reshape(6)
    eig, vec = np.zeros(3), np.zeros((3, 3))
    rc = load_library().lii_sym3_eigen(_ptr(m), _ptr(eig), _ptr(vec))
    if rc != 0:
        raise LIIError(rc, "lii_sym3_eigen")
    return eig, vec


class State:
    """StatesGroup (reference include/common_lib.h:68-169) as the 612-double `lii_state` POD."""

    def __init__(self, pod=None):
        if pod is None:
            pod = np.zeros(STATE_DOUBLES)
            pod[0:9] = np.eye(3).reshape(-1)
            pod[12:21] = np.eye(3).reshape(-1)
            cov = np.eye(24)
            cov[15:, 15:] = np.eye(9) * 0.00001  # INIT_COV, common_lib.h:79-80
            pod[36:] = cov.reshape(-1)
        self.pod = np.ascontiguousarray(pod, dtype=np.float64).copy()
        assert self.pod.shape == (STATE_DOUBLES,)

    def copy(self):
        return State(self.pod)

    rot_end = property(lambda s: s.pod[0:9].reshape(3, 3))
    pos_end = property(lambda s: s.pod[9:12])
    offset_R_L_I = property(lambda s: s.pod[12:21].reshape(3, 3))
    offset_T_L_I = property(lambda s: s.pod[21:24])
    vel_end = property(lambda s: s.pod[24:27])
    bias_g = property(lambda s: s.pod[27:30])
    bias_a = property(lambda s: s.pod[30:33])
    gravity = property(lambda s: s.pod[33:36])
    cov = property(lambda s: s.pod[36:].reshape(24, 24))


def scan_sorted_value(scan_sorted) -> int:
    """lii_scan_job::scan_sorted from the Python argument: False / 0 - nothing is assumed; True / 1 - ascending time order;
    2 / "sort" - the library sorts the scan by time on the device first."""
    if isinstance(scan_sorted, str):
        if scan_sorted != "sort":
            raise ValueError(f"scan_sorted: {scan_sorted!r} (False, True, 2 or 'sort')")
        return 2
    if not isinstance(scan_sorted, (bool, np.bool_)) and scan_sorted == 2:
        return 2
    return 1 if scan_sorted else 0


def _scan_job(undistort, imu_poses, leaf, max_iterations, imu_en, scan_dev, scan_sorted, map_update, next_scan, while_waiting):
    """A lii_scan_job of the current ABI, and the objects that must stay alive with it (the pose array, the WAIT_HOOK thunk)."""
    job = lii_scan_job()
    job.struct_size = C.sizeof(lii_scan_job)
    job.undistort = int(undistort)
    job.scan_sorted = scan_sorted_value(scan_sorted)
    job.map_update = 1 if map_update else 0
    if scan_dev is not None:
        job.scan_dev, job.n_scan_dev = scan_dev[0], scan_dev[1]
    if next_scan is not None:  # a device_scan() handle: the scan the NEXT call will bring (lii_scan_job::next_scan_dev - its prologue is pre-armed)
        job.next_scan_dev, job.next_n_scan = next_scan[0], next_scan[1]
    hook = None
    if while_waiting is not None:  # a Python callable: runs once inside the call, when every launch is enqueued (lii_scan_job::while_waiting)
        hook = WAIT_HOOK(lambda _arg: while_waiting())
        job.while_waiting = C.cast(hook, C.c_void_p)
    poses = None
    if imu_poses is not None:
        poses = np.ascontiguousarray(imu_poses, np.float64).reshape(-1, 22)
        job.imu_poses, job.n_imu_poses = _ptr(poses), len(poses)
    job.leaf = float(leaf)
    job.opts = lii_iekf_opts(int(max_iterations), int(imu_en))
    return job, (poses, hook)


def _report(rep):
    """The report dict of a lii_iekf_report."""
    return dict(iterations=rep.iterations, searches=rep.searches, effect_num=rep.effect_num,
                converged=bool(rep.converged), normal_eq=np.array(rep.normal_eq[:]))


def pose6d_array(n):
    """n x 22 doubles: offset_time, acc[3], gyr[3], vel[3], pos[3], rot[9] (msg/Pose6D.msg)."""
    return np.zeros((n, 22))


def calib_state_array(n):
    """n x 22 doubles: rot_end[9], ang_vel[3], linear_vel[3], ang_acc[3], linear_acc[3], timestamp."""
    a = np.zeros((n, 22))
    a[:, 0] = a[:, 4] = a[:, 8] = 1.0
    return a


def poses_array(poses):
    """Candidate poses as lii_pose_score takes them: (K, 12) float64, rot_end row-major then pos_end.  Accepts that array, or a pair
    (R (K, 3, 3), p (K, 3))."""
    if isinstance(poses, (tuple, list)) and len(poses) == 2 and np.ndim(poses[0]) == 3:
        R, p = np.asarray(poses[0], np.float64), np.asarray(poses[1], np.float64)
        return np.ascontiguousarray(np.concatenate([R.reshape(len(R), 9), p.reshape(len(R), 3)], axis=1))
    return np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 12))


def pose_grid(center_R, center_p, half_xy, step_xy, yaw_from, yaw_to, yaw_step):
    """Candidate poses around (center_R, center_p) - pure numpy: yaw-about-world-z variations of center_R at positions offset in x and y.
    Offsets: o_i = -half_xy + i step_xy for i = 0 .. floor(2 half_xy / step_xy + 1e-9) on each axis; yaws: yaw_from + j yaw_step while
    < yaw_to - 1e-9 (yaw_to is exclusive: 0 .. 2 pi lists every direction once).  Pose (ix, iy, j) is R = Rz(yaw_j) center_R,
    p = center_p + (o_ix, o_iy, 0) - roll, pitch and z are the centre's.  ORDER: x slowest, then y, yaw fastest - index
    (ix * ny + iy) * n_yaw + j.  Returns (R (K, 3, 3), p (K, 3)), float64.  A step that is not positive: ValueError."""
    if not (step_xy > 0 and yaw_step > 0 and half_xy >= 0 and np.isfinite([half_xy, step_xy, yaw_from, yaw_to, yaw_step]).all()):
        raise ValueError("pose_grid: step_xy and yaw_step must be positive, half_xy not negative, everything finite")
    center_R = np.asarray(center_R, np.float64).reshape(3, 3)
    center_p = np.asarray(center_p, np.float64).reshape(3)
    n_off = int(np.floor(2.0 * half_xy / step_xy + 1e-9)) + 1
    off = -float(half_xy) + float(step_xy) * np.arange(n_off)
    n_yaw = max(int(np.ceil((yaw_to - yaw_from) / yaw_step - 1e-9)), 0)
    yaws = float(yaw_from) + float(yaw_step) * np.arange(n_yaw)
    c, s = np.cos(yaws), np.sin(yaws)
    Rz = np.zeros((n_yaw, 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = c, -s, s, c, 1.0
    Ry = Rz @ center_R
    K = n_off * n_off * n_yaw
    R = np.broadcast_to(Ry, (n_off, n_off, n_yaw, 3, 3)).reshape(K, 3, 3).copy()
    p = np.empty((n_off, n_off, n_yaw, 3))
    p[..., 0] = center_p[0] + off[:, None, None]
    p[..., 1] = center_p[1] + off[None, :, None]
    p[..., 2] = center_p[2]
    return R, p.reshape(K, 3)


def rank_poses(effect_num, total_residual):
    """The ranking rule of Registrar.relocalize: indices by effect_num descending, then mean residual (total_residual / effect_num; +inf
    where nothing was selected) ascending, then index ascending."""
    eff = np.asarray(effect_num, np.int64)
    tot = np.asarray(total_residual, np.float64)
    mean = np.where(eff > 0, tot / np.maximum(eff, 1), np.inf)
    return np.lexsort((np.arange(len(eff)), mean, -eff))


# ---------------------------------------------------------------------- windows of an accumulation (Registrar.li_init_windows)
def li_init_window_array(windows):
    """Windows as an array of LI_INIT_WINDOW_IN_DTYPE: such an array as it is; rows (begin, count) - the aligned form, both
    sequences - or (imu_begin, imu_count, lidar_begin, lidar_count[, move_start_time])."""
    if isinstance(windows, np.ndarray) and windows.dtype == LI_INIT_WINDOW_IN_DTYPE:
        return np.ascontiguousarray(windows)
    rows = [tuple(w) for w in windows]
    out = np.zeros(len(rows), LI_INIT_WINDOW_IN_DTYPE)
    for k, w in enumerate(rows):
        if len(w) == 2:
            w = (w[0], w[1], w[0], w[1], 0.0)
        elif len(w) == 4:
            w = w + (0.0,)
        elif len(w) != 5:
            raise ValueError("a window is (begin, count) or (imu_begin, imu_count, lidar_begin, lidar_count[, move_start_time])")
        out[k] = w
    return out


def _imu_range(imu_t, t_from, t_to):
    """[begin, end) of the IMU stamps in [t_from, t_to] (ascending stamps)"""
    return int(np.searchsorted(imu_t, t_from, "left")), int(np.searchsorted(imu_t, t_to, "right"))


def li_init_prefix_windows(lidar_t, imu_t=None, first=200, step=50, margin=0.0, move_start_time=0.0):
    """The prefixes of an accumulation that the reference's loop (src/laserMapping.cpp:1190-1198) would have calibrated on had the
    initialisation fired at frame n: LiDAR [0, n) for n = first, first + step, ... and the whole accumulation last.
    imu_t = None: the aligned form (both sequences take the range; first >= 200).  Else the raw form: the IMU range of a window is
    [0, e) with e behind the last IMU stamp not later than the window's last LiDAR stamp plus `margin`; every window carries
    move_start_time.  Returns an array of LI_INIT_WINDOW_IN_DTYPE."""
    lidar_t = np.asarray(lidar_t, np.float64)
    n = len(lidar_t)
    if step < 1 or first < 1:
        raise ValueError("first and step must be positive")
    if imu_t is None and first < 200:
        raise ValueError("an aligned window holds 200 states or more")
    if first > n:
        raise ValueError("the accumulation is shorter than the first window")
    counts = list(range(first, n + 1, step))
    if counts[-1] != n:
        counts.append(n)
    out = np.zeros(len(counts), LI_INIT_WINDOW_IN_DTYPE)
    out["lidar_count"] = counts
    if imu_t is None:
        out["imu_count"] = counts
    else:
        imu_t = np.asarray(imu_t, np.float64)
        out["imu_count"] = [_imu_range(imu_t, -np.inf, lidar_t[c - 1] + margin)[1] for c in counts]
        out["move_start_time"] = move_start_time
    return out


def li_init_sliding_windows(lidar_t, imu_t=None, length=400, step=100, margin=0.0):
    """Windows of `length` LiDAR states every `step` states: LiDAR [b, b + length) for b = 0, step, ... while the window fits.
    imu_t = None: the aligned form (length >= 200).  Else the raw form: the IMU range of a window holds the stamps from the window's
    first LiDAR stamp minus `margin` to its last plus `margin`, and its move_start_time is its first LiDAR stamp (nothing of the
    window is older than move_start_time - 3 s).  Returns an array of LI_INIT_WINDOW_IN_DTYPE."""
    lidar_t = np.asarray(lidar_t, np.float64)
    n = len(lidar_t)
    if step < 1 or length < 1:
        raise ValueError("length and step must be positive")
    if imu_t is None and length < 200:
        raise ValueError("an aligned window holds 200 states or more")
    if length > n:
        raise ValueError("the accumulation is shorter than one window")
    begins = np.arange(0, n - length + 1, step)
    out = np.zeros(len(begins), LI_INIT_WINDOW_IN_DTYPE)
    out["lidar_begin"], out["lidar_count"] = begins, length
    if imu_t is None:
        out["imu_begin"], out["imu_count"] = begins, length
    else:
        imu_t = np.asarray(imu_t, np.float64)
        for k, b in enumerate(begins):
            lo, hi = _imu_range(imu_t, lidar_t[b] - margin, lidar_t[b + length - 1] + margin)
            out[k]["imu_begin"], out[k]["imu_count"] = lo, hi - lo
            out[k]["move_start_time"] = lidar_t[b]
    return out


def li_init_spread(records):
    """How far the calibrations of Registrar.li_init_windows lie apart.  Over the LII_WIN_OK records, against the last of them:
    the rotation angle of R_LI_w R_LI_last^T in degrees, |T_LI_w - T_LI_last| and total_time_lag_w - total_time_lag_last per
    window, and the mean and standard deviation of each.  Returns a dict: index (the OK records' positions), rot_deg, dT, dlag
    (arrays, one entry per OK record, the last one zero) and rot_deg_mean / _std, dT_mean / _std, dlag_mean / _std."""
    records = np.asarray(records)
    idx = np.flatnonzero(records["status"] == LII_WIN_OK)
    if len(idx) == 0:
        raise ValueError("no window came back LII_WIN_OK")
    ok = records[idx]
    last = ok[-1]
    D = ok["R_LI"] @ last["R_LI"].T
    # the angle from both the skew part and the trace: exact near 0 and near 180 degrees
    skew = 0.5 * np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], axis=1)
    rot = np.degrees(np.arctan2(np.linalg.norm(skew, axis=1), 0.5 * (np.trace(D, axis1=1, axis2=2) - 1.0)))
    out = dict(index=idx, rot_deg=rot, dT=np.linalg.norm(ok["T_LI"] - last["T_LI"], axis=1),
               dlag=ok["total_time_lag"] - last["total_time_lag"])
    for k in ("rot_deg", "dT", "dlag"):
        out[k + "_mean"], out[k + "_std"] = float(np.mean(out[k])), float(np.std(out[k]))
    return out


class Registrar:
    def __init__(self, max_scan_points=200_000, max_map_points=2_000_000, filter_size_map=0.15, map_cell_size=0.0,
                 device=0):
        self.L = load_library()
        n = C.c_int(0)
        rc = self.L.lii_device_count(C.byref(n))
        if rc != 0 or n.value <= 0:
            raise LIIError(-2, "no HIP device visible — libliinit_hip has no CPU fallback")
        cfg = lii_config()
        cfg.struct_size = C.sizeof(lii_config)
        cfg.device = device
        cfg.max_scan_points = int(max_scan_points)
        cfg.max_map_points = int(max_map_points)
        cfg.map_cell_size = float(map_cell_size)
        cfg.map_downsample_size = float(filter_size_map)
        cfg.max_match_dist2 = 5.0
        cfg.plane_threshold = 0.1
        cfg.laser_point_cov_inv = 1000.0
        self.h = C.c_void_p()
        self._check(self.L.lii_create(C.byref(cfg), C.byref(self.h)), None)
        self.max_scan_points = int(max_scan_points)
        self.max_map_points = int(max_map_points)
        self._dev_bufs = []

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc, h=True):
        if rc != 0:
            msg = self.L.lii_last_error(self.h if h else None)
            raise LIIError(rc, (msg or b"").decode() or self.L.lii_strerror(rc).decode())

    def close(self):
        if getattr(self, "h", None):
            for p in self._dev_bufs:
                self.L.lii_dev_free(self.h, p)
            self._dev_bufs = []
            self.L.lii_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._check(self.L.lii_synchronize(self.h))

    # ------------------------------------------------------------------ local map
    def map_reset(self):
        self._check(self.L.lii_map_reset(self.h))

    def map_build(self, xyz):
        xyz = np.ascontiguousarray(xyz, np.float32)
        self._check(self.L.lii_map_build(self.h, _ptr(xyz), len(xyz), xyz.strides[0]))

    @staticmethod
    def _xyzi_records(pts):
        """(array, stride, intensity offset) of an _xyzi input: (n, 4) float32 = x, y, z, intensity, or (n, 12) = pcl::PointXYZINormal."""
        pts = np.ascontiguousarray(pts, np.float32)
        assert pts.ndim == 2 and pts.shape[1] in (4, 12)
        return pts, (pts.strides[0] if len(pts) else 4 * pts.shape[1]), (12 if pts.shape[1] == 4 else 32)

    def map_build_xyzi(self, pts, stride_bytes=None, intensity_offset=None):
        """map_build with an intensity a point (lii_map_build_xyzi): pts (n, 4) = x, y, z, intensity, or (n, 12) = the 48-byte
        pcl::PointXYZINormal record (intensity at byte 32).  stride_bytes / intensity_offset override what the shape implies."""
        pts, stride, off = self._xyzi_records(pts)
        self._check(self.L.lii_map_build_xyzi(self.h, _ptr(pts) if len(pts) else None, len(pts), int(stride if stride_bytes is None else stride_bytes),
                                              int(off if intensity_offset is None else intensity_offset)))

    def map_intensity_set(self, on: bool):
        """lii_map_intensity_set: the scan-driven map updates (map_incremental, a registration's own map_update, map_build_from_scan) store
        each inserted point's intensity from the down-sampled cloud's; off by default."""
        self._check(self.L.lii_map_intensity_set(self.h, int(bool(on))))

    def map_intensity_get(self) -> bool:
        on = C.c_int32(0)
        self._check(self.L.lii_map_intensity_get(self.h, C.byref(on)))
        return bool(on.value)

    def map_build_from_scan(self, state: "State") -> int:
        """The first scan seeds the map (src/laserMapping.cpp:921-929): the current down-sampled cloud, moved to the world frame at
        `state` on the device, becomes the map (lii_map_build_from_scan).  Returns the number of map points (0: five points or
        fewer, nothing built)."""
        n = C.c_int32(0)
        self._check(self.L.lii_map_build_from_scan(self.h, _ptr(state.pod), C.byref(n)))
        return n.value

    def map_add_points(self, xyz, downsample_on: bool) -> int:
        xyz = np.ascontiguousarray(xyz, np.float32)
        n = C.c_int32(0)
        self._check(self.L.lii_map_add_points(self.h, _ptr(xyz), len(xyz), xyz.strides[0] if len(xyz) else 12,
                                              int(downsample_on), C.byref(n)))
        return n.value

    def map_add_points_xyzi(self, pts, downsample_on: bool, stride_bytes=None, intensity_offset=None) -> int:
        """map_add_points with an intensity a point (lii_map_add_points_xyzi; records as for map_build_xyzi): the stored point keeps the
        intensity of the input point the keep-closest-to-centre rule keeps."""
        pts, stride, off = self._xyzi_records(pts)
        n = C.c_int32(0)
        self._check(self.L.lii_map_add_points_xyzi(self.h, _ptr(pts) if len(pts) else None, len(pts), int(stride if stride_bytes is None else stride_bytes),
                                                   int(off if intensity_offset is None else intensity_offset), int(downsample_on), C.byref(n)))
        return n.value

    def map_delete_boxes(self, boxes6) -> int:
        """ikdtree.Delete_Point_Boxes: boxes6 (n, 6) = min xyz, max xyz; returns the number of points removed."""
        b = np.ascontiguousarray(boxes6, np.float32).reshape(-1, 6)
        n = C.c_int32(0)
        self._check(self.L.lii_map_delete_boxes(self.h, _ptr(b) if len(b) else None, len(b), C.byref(n)))
        return n.value

    def map_delete_points(self, xyz) -> int:
        """ikdtree.Delete_Points: every row of xyz (n, >= 3) takes ONE live stored point that same_point accepts (1e-6 an axis) out of the
        map - a list that holds a point c times removes min(c, stored copies); returns the number of points removed."""
        q = np.asarray(xyz, np.float32)
        if q.ndim != 2 or q.shape[1] < 3 or not q.flags.c_contiguous:
            q = np.ascontiguousarray(q.reshape(-1, q.shape[-1])[:, :3] if q.ndim >= 2 else q.reshape(-1, 3))
        n = C.c_int32(0)
        self._check(self.L.lii_map_delete_points(self.h, _ptr(q) if len(q) else None, len(q), q.strides[0] if len(q) else 12, C.byref(n)))
        return n.value

    def map_delete_points_dev(self, q_dev, n, stride_bytes=12):
        """map_delete_points with the list in device memory the caller owns - a raw address or an object with __cuda_array_interface__
        (a torch tensor): float xyz every stride_bytes.  Enqueued on the handle's stream; map_size() behind it reads the result."""
        self._check(self.L.lii_map_delete_points_dev(self.h, _dev_address(q_dev), int(n), int(stride_bytes)))

    def map_range(self):
        """ikdtree.tree_range(): (6,) float32 - the exact min xyz, max xyz of the live points; zeros for an empty map."""
        r = (C.c_float * 6)()
        self._check(self.L.lii_map_range(self.h, r))
        return np.array(r, np.float32)

    def map_box_search(self, boxes6):
        """ikdtree.Search_by_range for boxes6 (n, 6) = min xyz, max xyz: the live points with min <= p < max in at least one box, each
        once, as (m, 3) float32 in no particular order.  Leaves the handle's neighbour lists and everything else of a registration alone."""
        b = np.ascontiguousarray(boxes6, np.float32).reshape(-1, 6)
        n = C.c_int32(0)
        self._check(self.L.lii_map_box_search(self.h, _ptr(b) if len(b) else None, len(b), None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 3), np.float32)
        self._check(self.L.lii_map_box_search(self.h, _ptr(b) if len(b) else None, len(b), _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    def map_box_search_xyzi(self, boxes6):
        """map_box_search as (m, 4) float32: x, y, z and the stored intensity."""
        b = np.ascontiguousarray(boxes6, np.float32).reshape(-1, 6)
        n = C.c_int32(0)
        self._check(self.L.lii_map_box_search_xyzi(self.h, _ptr(b) if len(b) else None, len(b), None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 4), np.float32)
        self._check(self.L.lii_map_box_search_xyzi(self.h, _ptr(b) if len(b) else None, len(b), _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    # ---- the moving local map (lasermap_fov_segment + the box delete upstream never made)
    @staticmethod
    def _local_map_info(info) -> dict:
        nb = int(info.last_n_boxes)
        return {"initialized": bool(info.initialized), "cube": np.array(info.cube, np.float32), "n_boxes": nb,
                "boxes": np.array(info.last_boxes, np.float32).reshape(3, 6)[:nb].copy(), "n_deleted": int(info.last_n_deleted),
                "moves": int(info.moves), "deleted_total": int(info.deleted_total)}

    def local_map_set(self, cube_len, det_range, enabled=True):
        """lii_local_map_set: the cube's edge and the detection range; enabled: every scan_register* call segments by itself.
        Every call starts the cube over (Localmap_Initialized = false)."""
        o = lii_local_map_opts(C.sizeof(lii_local_map_opts), int(bool(enabled)), float(cube_len), float(det_range), 0)
        self._check(self.L.lii_local_map_set(self.h, C.byref(o)))

    def local_map_get(self) -> dict:
        """The cube and what the last call that ran did (waits for the stream)."""
        info = lii_local_map_info()
        self._check(self.L.lii_local_map_get(self.h, C.byref(info)))
        return self._local_map_info(info)

    def local_map_segment(self, pos_end, report=True):
        """One lasermap_fov_segment at pos_end (state.pos_end) + the delete of its boxes; report=False only enqueues."""
        p = (C.c_double * 3)(*[float(x) for x in np.asarray(pos_end, np.float64).reshape(3)])
        if not report:
            self._check(self.L.lii_local_map_segment(self.h, p, None))
            return None
        info = lii_local_map_info()
        self._check(self.L.lii_local_map_segment(self.h, p, C.byref(info)))
        return self._local_map_info(info)

    # ---- the history of what box deletes remove (points_cache_collect / acquire_removed_points)
    def map_removed_set(self, capacity):
        """lii_map_removed_set: a device buffer of `capacity` points that every box delete appends its points to; 0: off (the contents stay
        readable), the same capacity again: contents kept, another: a new, empty buffer."""
        self._check(self.L.lii_map_removed_set(self.h, int(capacity)))

    def map_removed_get(self) -> dict:
        """capacity (0: off), held, collected_total, lost_total (waits for the stream)."""
        info = lii_map_removed_info(C.sizeof(lii_map_removed_info))
        self._check(self.L.lii_map_removed_get(self.h, C.byref(info)))
        return {"capacity": int(info.capacity), "held": int(info.held), "collected_total": int(info.collected_total),
                "lost_total": int(info.lost_total)}

    def map_removed_acquire(self, clear=False, strict=True):
        """The history buffer as (n, 3) float32, in no particular order; clear: the buffer is empty afterwards.  A buffer that overflowed
        raises LIIError(-4) BEFORE anything is delivered or cleared; strict=False delivers what it holds instead."""
        n = C.c_int32(0)
        rc = self.L.lii_map_removed_acquire(self.h, None, 0, C.byref(n), 0)  # (the count; -4: overflowed - nothing is cleared by this form)
        if rc != 0 and (strict or rc != -4):
            self._check(rc)
        out = np.zeros((max(n.value, 1), 3), np.float32)
        rc = self.L.lii_map_removed_acquire(self.h, _ptr(out), len(out), C.byref(n), int(bool(clear)))
        if rc != 0 and (strict or rc != -4):
            self._check(rc)
        return out[:n.value]

    def map_removed_acquire_xyzi(self, clear=False, strict=True):
        """map_removed_acquire as (n, 4) float32: x, y, z and the intensity the point was stored with."""
        n = C.c_int32(0)
        rc = self.L.lii_map_removed_acquire_xyzi(self.h, None, 0, C.byref(n), 0)
        if rc != 0 and (strict or rc != -4):
            self._check(rc)
        out = np.zeros((max(n.value, 1), 4), np.float32)
        rc = self.L.lii_map_removed_acquire_xyzi(self.h, _ptr(out), len(out), C.byref(n), int(bool(clear)))
        if rc != 0 and (strict or rc != -4):
            self._check(rc)
        return out[:n.value]

    def map_removed_view(self):
        """(device float4 records as an object with __cuda_array_interface__ - torch.as_tensor(v, device="cuda") -, n); valid until the next
        call that deletes or clears.  n == 0: (None, 0)."""
        p, n = C.c_void_p(), C.c_int32(0)
        self._check(self.L.lii_map_removed_view(self.h, C.byref(p), C.byref(n)))
        if n.value == 0 or not p.value:
            return None, 0
        return _DeviceFloat4(p.value, n.value), n.value

    def global_map(self):
        """Everything the run has mapped, at map resolution: the history (acquired, not cleared) followed by map_download()."""
        return np.concatenate([self.map_removed_acquire(clear=False), self.map_download()])

    def map_size(self) -> int:
        n = C.c_int32(0)
        self._check(self.L.lii_map_size(self.h, C.byref(n)))
        return n.value

    def map_download(self):
        n = C.c_int32(0)
        self._check(self.L.lii_map_download(self.h, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 3), np.float32)
        self._check(self.L.lii_map_download(self.h, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    def map_download_xyzi(self):
        """map_download as (n, 4) float32: x, y, z and the stored intensity (0.0 for points that came without one)."""
        n = C.c_int32(0)
        self._check(self.L.lii_map_download_xyzi(self.h, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 4), np.float32)
        self._check(self.L.lii_map_download_xyzi(self.h, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    def map_pcd(self):
        """lii_map_pcd: the live map as the 32-byte rows pcd_header(n) describes (normals and curvature 0, intensity the stored word):
        (n, 32) uint8; pcd_header(len(rows)) + rows.tobytes() is the file."""
        n = C.c_int32(0)
        self._check(self.L.lii_map_pcd(self.h, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 32), np.uint8)
        self._check(self.L.lii_map_pcd(self.h, _ptr(out), out.nbytes, C.byref(n)))
        return out[:n.value]

    def map_commit(self):
        self._check(self.L.lii_map_commit(self.h))

    def map_nearest(self, q, k=5, max_dist=5.0):
        """ikdtree.Nearest_Search for the points q (n, >= 3) float: the min(k, m) nearest of the m map points with d2 <= max_dist
        (the SQUARED distance against max_dist, as the reference compares), ascending.  Returns (pts (n, k, 3), d2 (n, k), count (n,));
        the rows from count[i] on are zeros.  Leaves the handle's scan, neighbour lists and everything else of a registration alone."""
        q = np.asarray(q, np.float32)
        if q.ndim != 2 or q.shape[1] < 3 or not q.flags.c_contiguous:
            q = np.ascontiguousarray(q.reshape(-1, q.shape[-1])[:, :3] if q.ndim >= 2 else q.reshape(-1, 3))
        n, k = len(q), int(k)
        pts = np.zeros((n, max(k, 0), 3), np.float32)
        d2 = np.zeros((n, max(k, 0)), np.float32)
        cnt = np.zeros(n, np.int32)
        self._check(self.L.lii_map_nearest(self.h, _ptr(q) if n else None, n, q.strides[0] if n else 12, k, float(max_dist),
                                           _ptr(pts), _ptr(d2), _ptr(cnt)))
        return pts, d2, cnt

    def map_nearest_xyzi(self, q, k=5, max_dist=5.0):
        """map_nearest with 4 floats a row: (pts (n, k, 4) = x, y, z, intensity, d2 (n, k), count (n,))."""
        q = np.asarray(q, np.float32)
        if q.ndim != 2 or q.shape[1] < 3 or not q.flags.c_contiguous:
            q = np.ascontiguousarray(q.reshape(-1, q.shape[-1])[:, :3] if q.ndim >= 2 else q.reshape(-1, 3))
        n, k = len(q), int(k)
        pts = np.zeros((n, max(k, 0), 4), np.float32)
        d2 = np.zeros((n, max(k, 0)), np.float32)
        cnt = np.zeros(n, np.int32)
        self._check(self.L.lii_map_nearest_xyzi(self.h, _ptr(q) if n else None, n, q.strides[0] if n else 12, k, float(max_dist),
                                                _ptr(pts), _ptr(d2), _ptr(cnt)))
        return pts, d2, cnt

    def dev_alloc(self, nbytes: int) -> int:
        """nbytes of device memory of the library's (lii_dev_alloc), released with the Registrar; returns the address."""
        p = C.c_void_p()
        self._check(self.L.lii_dev_alloc(self.h, max(int(nbytes), 16), C.byref(p)))
        self._dev_bufs.append(p)
        return int(p.value)

    def dev_upload(self, dev_ptr, a):
        """Copies the bytes of array `a` to device memory at `dev_ptr` (dev_alloc); synchronous (lii_dev_upload)."""
        a = np.ascontiguousarray(a)
        if a.nbytes:
            self._check(self.L.lii_dev_upload(self.h, C.c_void_p(_dev_address(dev_ptr)), _ptr(a), a.nbytes))

    def map_nearest_dev(self, q_dev, n, k, max_dist, pts_dev, d2_dev, count_dev, stride_bytes=12):
        """map_nearest with queries and results in device memory the caller owns - raw addresses, or objects with
        __cuda_array_interface__ (torch tensors): float xyz every stride_bytes in, (n, k, 3) float32 / (n, k) float32 / (n,) int32 out
        (pts_dev / d2_dev may be None).  Enqueued on the handle's stream; synchronize() - or any synchronous call - orders it."""
        self._check(self.L.lii_map_nearest_dev(self.h, _dev_address(q_dev), int(n), int(stride_bytes), int(k), float(max_dist),
                                               _dev_address(pts_dev), _dev_address(d2_dev), _dev_address(count_dev)))

    def map_nearest_xyzi_dev(self, q_dev, n, k, max_dist, pts_dev, d2_dev, count_dev, stride_bytes=12):
        """map_nearest_dev with (n, k, 4) float32 rows: x, y, z, intensity."""
        self._check(self.L.lii_map_nearest_xyzi_dev(self.h, _dev_address(q_dev), int(n), int(stride_bytes), int(k), float(max_dist),
                                                    _dev_address(pts_dev), _dev_address(d2_dev), _dev_address(count_dev)))

    # ------------------------------------------------------------------ candidate poses against the map
    def pose_score(self, base: State, poses, want_res=False):
        """lii_pose_score: the figures of one search pass (src/laserMapping.cpp:957-1020, all-true selection) of the current
        down-sampled cloud at each of the K poses - `poses` is (K, 12) doubles, rot_end row-major then pos_end, or a pair (R (K, 3, 3),
        p (K, 3)) as pose_grid returns it; the extrinsic is base's.  Returns (n_full int32 (K,), effect_num int32 (K,), total_residual
        float64 (K,)) and, with want_res, res float32 (K, n_down): |pd2| of a selected point, -1000 otherwise.  Leaves the neighbour
        lists, the selection and everything else of a registration alone."""
        P = poses_array(poses)
        K = len(P)
        sc = np.zeros(K, POSE_SCORE_DTYPE)
        res = None
        if want_res:
            n = C.c_int32(0)
            self._check(self.L.lii_scan_download(self.h, 1, None, 0, C.byref(n)))  # (the size of the down-sampled cloud)
            res = np.zeros((K, n.value), np.float32)
        self._check(self.L.lii_pose_score(self.h, _ptr(base.pod), _ptr(P) if K else None, K, _ptr(sc) if K else None,
                                          _ptr(res) if res is not None and res.size else None))
        out = (sc["n_full"].copy(), sc["effect_num"].copy(), sc["total_residual"].copy())
        return out + (res,) if want_res else out

    def pose_score_dev(self, base: State, poses_dev, n_poses, scores_dev, res_dev=None):
        """pose_score with poses, scores (16-byte struct lii_pose_score records) and res in device memory the caller owns - raw
        addresses or objects with __cuda_array_interface__; res rows in the device's order of the down-sampled cloud.  Enqueued on
        the handle's stream; synchronize() - or any synchronous call - orders it."""
        self._check(self.L.lii_pose_score_dev(self.h, _ptr(base.pod), _dev_address(poses_dev), int(n_poses), _dev_address(scores_dev),
                                              _dev_address(res_dev)))

    @staticmethod
    def _prior_ptr(prior_cov):
        if prior_cov is None:
            return None, None
        pc = np.ascontiguousarray(np.asarray(prior_cov, np.float64).reshape(6, 6))
        return pc, _ptr(pc)

    def pose_refine(self, base: State, poses, max_iterations=4, updates=2, prior_cov=None):
        """lii_pose_refine: the iterated update in LO mode (src/laserMapping.cpp:957-1134, imu_en = False) on the six pose states, `updates`
        times in a row from each of the K poses - `poses` as pose_score takes them; the extrinsic is base's - in ONE call: every round is
        enqueued at once, one wait.  prior_cov: the 6 x 6 covariance every pose starts from; None: the pose block of base.cov.  Returns a
        structured array (POSE_REFINED_DTYPE): pose (12), cov (6, 6), total_residual, effect_num, iterations, searches, flags.  Leaves the
        neighbour lists, the selection and everything else of a registration alone."""
        P = poses_array(poses)
        K = len(P)
        out = np.zeros(K, POSE_REFINED_DTYPE)
        pc, pc_ptr = self._prior_ptr(prior_cov)
        self._check(self.L.lii_pose_refine(self.h, _ptr(base.pod), pc_ptr, _ptr(P) if K else None, K, int(max_iterations), int(updates),
                                           _ptr(out) if K else None))
        return out

    def pose_refine_dev(self, base: State, poses_dev, n_poses, out_dev, max_iterations=4, updates=2, prior_cov=None):
        """pose_refine with poses and records (408-byte struct lii_pose_refined) in device memory the caller owns - raw addresses or
        objects with __cuda_array_interface__; prior_cov stays host memory.  Enqueued on the handle's stream; synchronize() - or any
        synchronous call - orders it."""
        pc, pc_ptr = self._prior_ptr(prior_cov)
        self._check(self.L.lii_pose_refine_dev(self.h, _ptr(base.pod), pc_ptr, _dev_address(poses_dev), int(n_poses), int(max_iterations),
                                               int(updates), _dev_address(out_dev)))

    def relocalize(self, base: State, poses, top=3, max_iterations=4, updates=2, batched=False):
        """Re-localisation over candidate poses: pose_score ranks them (rank_poses: effect_num descending, mean residual ascending, index),
        the `top` best each start `updates` consecutive iekf_update calls in LO mode (imu_en = False) on a copy of `base` with that pose,
        and the state whose last update selected the most points wins (the earlier rank on a tie).  Returns (state, info) with info =
        dict(order, n_full, effect_num, total_residual, tried = [(pose index, effect_num after its updates)], best = pose index).
        batched=True: the `top` best go through ONE pose_refine call instead - the registration state of the handle is left alone - and
        the returned state is `base` with the winning pose and its pose-covariance block."""
        P = poses_array(poses)
        n_full, effect, total = self.pose_score(base, P)
        order = rank_poses(effect, total)
        best, best_eff, best_k, tried = None, -1, -1, []
        if batched:
            cand = order[:max(int(top), 1)]
            rec = self.pose_refine(base, P[cand], max_iterations=max_iterations, updates=max(int(updates), 1))
            for k, r in zip(cand, rec):
                tried.append((int(k), int(r["effect_num"])))
                if r["effect_num"] > best_eff:
                    best_eff, best_k, win = int(r["effect_num"]), int(k), r
            best = base.copy()
            best.rot_end[:] = win["pose"][:9].reshape(3, 3)
            best.pos_end[:] = win["pose"][9:]
            best.cov[:6, :6] = win["cov"]
            return best, dict(order=order, n_full=n_full, effect_num=effect, total_residual=total, tried=tried, best=best_k)
        for k in order[:max(int(top), 1)]:
            st = base.copy()
            st.rot_end[:] = P[k, :9].reshape(3, 3)
            st.pos_end[:] = P[k, 9:]
            eff = 0
            for _ in range(max(int(updates), 1)):
                eff = self.iekf_update(st, st.copy(), max_iterations=max_iterations, imu_en=False)["effect_num"]
            tried.append((int(k), int(eff)))
            if eff > best_eff:
                best, best_eff, best_k = st, eff, int(k)
        return best, dict(order=order, n_full=n_full, effect_num=effect, total_residual=total, tried=tried, best=best_k)

    def map_radius(self, q, max_dist, sorted=False, points=True):
        """The ball query (upstream ikd-Tree's Radius_Search) for the points q (n, >= 3) float: EVERY map point with d2 <= max_dist
        (the SQUARED distance against max_dist, inclusive), however many there are.  Returns (offsets int64 (n + 1,), pts float32
        (total, 3), d2 float32 (total,)): the points of query i are rows offsets[i] .. offsets[i + 1] - 1, in the library's visiting
        order, or ascending in d2 with sorted=True.  points=False: the offsets only (pts and d2 come back empty).  A count-only call,
        then a call sized by its total.  Leaves the handle's scan, neighbour lists and everything else of a registration alone."""
        q = np.asarray(q, np.float32)
        if q.ndim != 2 or q.shape[1] < 3 or not q.flags.c_contiguous:
            q = np.ascontiguousarray(q.reshape(-1, q.shape[-1])[:, :3] if q.ndim >= 2 else q.reshape(-1, 3))
        n = len(q)
        flags = LII_RADIUS_SORTED if sorted else 0
        qp, stride = (_ptr(q) if n else None), (q.strides[0] if n else 12)
        offsets = np.zeros(n + 1, np.int64)
        total = C.c_int64(0)
        self._check(self.L.lii_map_radius(self.h, qp, n, stride, float(max_dist), flags, _ptr(offsets), None, None, 0, C.byref(total)))
        rows = total.value if points else 0
        pts = np.zeros((rows, 3), np.float32)
        d2 = np.zeros(rows, np.float32)
        if rows:
            self._check(self.L.lii_map_radius(self.h, qp, n, stride, float(max_dist), flags, _ptr(offsets), _ptr(pts), _ptr(d2), rows, C.byref(total)))
        return offsets, pts, d2

    def map_radius_dev(self, q_dev, n, max_dist, offsets_dev, pts_dev, d2_dev, capacity, total_dev, sorted=False, stride_bytes=12):
        """map_radius with queries and results in device memory the caller owns - raw addresses, or objects with
        __cuda_array_interface__ (torch tensors): float xyz every stride_bytes in; (n + 1,) int64 offsets, (capacity, 3) float32,
        (capacity,) float32 and one int64 total out (pts_dev / d2_dev may be None).  Rows with index >= capacity are not written: compare
        the total with the capacity behind synchronize().  Enqueued on the handle's stream."""
        self._check(self.L.lii_map_radius_dev(self.h, _dev_address(q_dev), int(n), int(stride_bytes), float(max_dist),
                                              LII_RADIUS_SORTED if sorted else 0, _dev_address(offsets_dev), _dev_address(pts_dev),
                                              _dev_address(d2_dev), int(capacity), _dev_address(total_dev)))

    def map_surface(self, q, max_dist, viewpoint=None):
        """The surface the map holds at the points q (n, >= 3) float: for each, the ball of map_radius(q, max_dist) reduced on the
        device to a record of SURFACE_DTYPE - count (the ball's population), valid (count >= 3), mean (the ball's centroid), eig (the
        covariance's eigenvalues, ascending), normal (unit, of eig[0]) and curvature (eig[0] / sum).  viewpoint (3,): the normals look at
        it; None: their largest component is positive.  Leaves everything of a registration alone."""
        q = np.asarray(q, np.float32)
        if q.ndim != 2 or q.shape[1] < 3 or not q.flags.c_contiguous:
            q = np.ascontiguousarray(q.reshape(-1, q.shape[-1])[:, :3] if q.ndim >= 2 else q.reshape(-1, 3))
        n = len(q)
        vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float64).reshape(3)
        out = np.zeros(n, SURFACE_DTYPE)
        self._check(self.L.lii_map_surface(self.h, _ptr(q) if n else None, n, q.strides[0] if n else 12, float(max_dist),
                                           None if vp is None else _ptr(vp), _ptr(out) if n else None))
        return out

    def map_surface_dev(self, q_dev, n, max_dist, out_dev, viewpoint=None, stride_bytes=12):
        """map_surface with queries and the n 88-byte records in device memory the caller owns (raw addresses or objects with
        __cuda_array_interface__); viewpoint stays a host array.  Enqueued on the handle's stream."""
        vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float64).reshape(3)
        self._check(self.L.lii_map_surface_dev(self.h, _dev_address(q_dev), int(n), int(stride_bytes), float(max_dist),
                                               None if vp is None else _ptr(vp), _dev_address(out_dev)))

    def map_crispness(self, max_dist, min_count=5, every=1):
        """How crisp is the map?  Mean map entropy (mme), mean plane variance (mpv) and mean ball population (mean_count) over the
        map's own points with hash % every == 0 whose ball of squared radius max_dist holds >= min_count points and is not degenerate;
        n_selected = n_used + n_sparse + n_degenerate.  Computed on the device, nothing is downloaded.  Returns a dict."""
        out = lii_map_crispness()
        self._check(self.L.lii_map_crispness(self.h, float(max_dist), int(min_count), int(every), C.byref(out)))
        return {name: getattr(out, name) for name, _ in lii_map_crispness._fields_}

    def map_radius_xyzi(self, q, max_dist, sorted=False, points=True):
        """map_radius with 4 floats a row: (offsets, pts (total, 4) = x, y, z, intensity, d2 (total,))."""
        q = np.asarray(q, np.float32)
        if q.ndim != 2 or q.shape[1] < 3 or not q.flags.c_contiguous:
            q = np.ascontiguousarray(q.reshape(-1, q.shape[-1])[:, :3] if q.ndim >= 2 else q.reshape(-1, 3))
        n = len(q)
        flags = LII_RADIUS_SORTED if sorted else 0
        qp, stride = (_ptr(q) if n else None), (q.strides[0] if n else 12)
        offsets = np.zeros(n + 1, np.int64)
        total = C.c_int64(0)
        self._check(self.L.lii_map_radius_xyzi(self.h, qp, n, stride, float(max_dist), flags, _ptr(offsets), None, None, 0, C.byref(total)))
        rows = total.value if points else 0
        pts = np.zeros((rows, 4), np.float32)
        d2 = np.zeros(rows, np.float32)
        if rows:
            self._check(self.L.lii_map_radius_xyzi(self.h, qp, n, stride, float(max_dist), flags, _ptr(offsets), _ptr(pts), _ptr(d2), rows, C.byref(total)))
        return offsets, pts, d2

    def map_radius_xyzi_dev(self, q_dev, n, max_dist, offsets_dev, pts_dev, d2_dev, capacity, total_dev, sorted=False, stride_bytes=12):
        """map_radius_dev with (capacity, 4) float32 rows: x, y, z, intensity."""
        self._check(self.L.lii_map_radius_xyzi_dev(self.h, _dev_address(q_dev), int(n), int(stride_bytes), float(max_dist),
                                                   LII_RADIUS_SORTED if sorted else 0, _dev_address(offsets_dev), _dev_address(pts_dev),
                                                   _dev_address(d2_dev), int(capacity), _dev_address(total_dev)))

    # ------------------------------------------------------------------ scan
    def scan_upload(self, pts):
        """pts: (n,4) float32 (x,y,z,t_ms) or a structured/2-D array with the 48-byte PointXYZINormal layout (n,12)."""
        pts = np.ascontiguousarray(pts, np.float32)
        assert pts.ndim == 2 and pts.shape[1] in (4, 12)
        toff = 12 if pts.shape[1] == 4 else 36
        self._check(self.L.lii_scan_upload(self.h, _ptr(pts), len(pts), pts.strides[0] if len(pts) else 16, toff))

    def scan_upload_next(self, pts):
        """Starts the NEXT scan on its way (copy stream, second device buffer); `pts` must stay alive and untouched until
        scan_advance() has returned (a pinned (n,4) source is read by the copy engine directly)."""
        assert pts.dtype == np.float32 and pts.flags.c_contiguous and pts.ndim == 2 and pts.shape[1] in (4, 12)
        toff = 12 if pts.shape[1] == 4 else 36
        self._check(self.L.lii_scan_upload_next(self.h, _ptr(pts), len(pts), pts.strides[0] if len(pts) else 16, toff))

    def scan_advance(self):
        """The scan handed to scan_upload_next becomes the current one (as scan_upload would have made it)."""
        self._check(self.L.lii_scan_advance(self.h))

    def device_scan(self, pts4):
        """Copies a float4 scan into a caller-owned device buffer; returns an opaque (ptr, n) for scan_set_device."""
        pts4 = np.ascontiguousarray(pts4, np.float32)
        assert pts4.ndim == 2 and pts4.shape[1] == 4
        p = C.c_void_p()
        self._check(self.L.lii_dev_alloc(self.h, max(pts4.nbytes, 16), C.byref(p)))
        self._dev_bufs.append(p)
        if len(pts4):
            self._check(self.L.lii_dev_upload(self.h, p, _ptr(pts4), pts4.nbytes))
        return (p, len(pts4))

    def scan_set_device(self, dev):
        self._check(self.L.lii_scan_set_device(self.h, dev[0], dev[1]))

    def scan_sort(self):
        """The current scan is put into ascending time order on the device (lii_scan_sort): stable, -0.0 and +0.0 equal - the
        reference's order.  scan_download(0) then returns the sorted scan and a registration may say scan_sorted=True."""
        self._check(self.L.lii_scan_sort(self.h))

    def undistort_imu(self, poses22, end_R, end_p, R_LI, T_LI):
        poses = np.ascontiguousarray(poses22, np.float64).reshape(-1, 22)
        a = [np.ascontiguousarray(x, np.float64).reshape(-1) for x in (end_R, end_p, R_LI, T_LI)]
        self._check(self.L.lii_undistort_imu(self.h, _ptr(poses), len(poses), *[_ptr(x) for x in a]))

    def undistort_cv(self, omega, vel, end_R):
        a = [np.ascontiguousarray(x, np.float64).reshape(-1) for x in (omega, vel, end_R)]
        self._check(self.L.lii_undistort_cv(self.h, *[_ptr(x) for x in a]))

    def downsample(self, leaf: float, want_count: bool = True):
        """Voxel-grid filter.  want_count=False keeps it asynchronous: the size of the result stays on the device
        (the registration kernels read it there) and no host synchronisation happens."""
        if not want_count:
            self._check(self.L.lii_downsample(self.h, float(leaf), None, None))
            return None
        n, f = C.c_int32(0), C.c_int32(0)
        self._check(self.L.lii_downsample(self.h, float(leaf), C.byref(n), C.byref(f)))
        return n.value, bool(f.value)

    def downsample_skip(self) -> int:
        n = C.c_int32(0)
        self._check(self.L.lii_downsample_skip(self.h, C.byref(n)))
        return n.value

    def scan_download(self, which=0):
        n = C.c_int32(0)
        self._check(self.L.lii_scan_download(self.h, which, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 4), np.float32)
        self._check(self.L.lii_scan_download(self.h, which, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    # ------------------------------------------------------------------ the intensity channel (optional; off until asked for)
    def scan_intensity_upload(self, intensity):
        """Attaches intensities to the current scan: (n,) float32, or the (n, 12) PointXYZINormal records (column 8)."""
        a = np.ascontiguousarray(intensity, np.float32)
        assert a.ndim == 1 or (a.ndim == 2 and a.shape[1] == 12)
        off = 0 if a.ndim == 1 else 32
        self._check(self.L.lii_scan_intensity_upload(self.h, _ptr(a), len(a), a.strides[0] if len(a) else 4, off))

    def device_intensity(self, intensity):
        """Copies (n,) float32 into a caller-owned device buffer; returns an opaque (ptr, n) for scan_intensity_set_device."""
        a = np.ascontiguousarray(intensity, np.float32).reshape(-1)
        p = C.c_void_p()
        self._check(self.L.lii_dev_alloc(self.h, max(a.nbytes, 16), C.byref(p)))
        self._dev_bufs.append(p)
        if len(a):
            self._check(self.L.lii_dev_upload(self.h, p, _ptr(a), a.nbytes))
        return (p, len(a))

    def scan_intensity_set_device(self, dev):
        self._check(self.L.lii_scan_intensity_set_device(self.h, dev[0], dev[1]))

    def ingest_set_intensity(self, on=True):
        """The standing order: every ingest call from now on also forms its frames' intensities; frame_select attaches them."""
        self._check(self.L.lii_ingest_set_intensity(self.h, int(bool(on))))

    def ingest_set_features(self, on=True):
        """The standing order (preprocess/feature_extract_en; `on` may be Params.feature_extract_en): a whole-message ingest
        (cut_frame_num = 0) of AVIA, VELO or OUSTER returns ONE frame holding the feature branch's pl_surf; ingest_corners gives pl_corn."""
        self._check(self.L.lii_ingest_set_features(self.h, int(bool(on))))

    def ingest_corners(self):
        """pl_corn of the message whose frames are current: ((n, 4) float32 x y z curvature, (n,) float32 intensity)."""
        n = C.c_int32(0)
        self._check(self.L.lii_ingest_corners_download(self.h, None, None, 0, C.byref(n)))
        xyzt = np.zeros((max(n.value, 1), 4), np.float32)
        inten = np.zeros(max(n.value, 1), np.float32)
        self._check(self.L.lii_ingest_corners_download(self.h, _ptr(xyzt), _ptr(inten), len(xyzt), C.byref(n)))
        return xyzt[:n.value], inten[:n.value]

    def ingest_features(self):
        """dict(on, n_surf, n_corn, n_lines): the order, and the counts of the message whose frames are current."""
        v = [C.c_int32(0) for _ in range(4)]
        self._check(self.L.lii_ingest_features_get(self.h, *[C.byref(x) for x in v]))
        return dict(on=bool(v[0].value), n_surf=v[1].value, n_corn=v[2].value, n_lines=v[3].value)

    def scan_intensity_download(self, which=0):
        """which=0: the current scan's intensities; 1: the down-sampled cloud's, in the order scan_download(1) returns its points."""
        n = C.c_int32(0)
        self._check(self.L.lii_scan_intensity_download(self.h, which, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.float32)
        self._check(self.L.lii_scan_intensity_download(self.h, which, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    # ------------------------------------------------------------------ ingest
    def _ingest(self, fn, data, n_points, fields, lidar_type, n_scans, point_filter_num, blind, stamp_s, cut_frame_num,
                scan_count):
        raw = np.frombuffer(data, np.uint8)
        opts = lii_ingest_opts(C.sizeof(lii_ingest_opts), lidar_type, n_scans, point_filter_num, blind, stamp_s,
                               cut_frame_num, scan_count)
        frames = (lii_frame_info * 64)()
        nf = C.c_int32(0)
        self._check(fn(self.h, _ptr(raw) if len(raw) else None, n_points, C.byref(fields), C.byref(opts), frames, 64, C.byref(nf)))
        self.frame_tail_ms = [frames[k].last_offset_ms for k in range(nf.value)]  # curvature of each frame's last point
        return [(frames[k].begin_time_s, frames[k].offset, frames[k].count) for k in range(nf.value)]

    def ingest_pcl2(self, data, n_points, fields, lidar_type, n_scans, point_filter_num, blind, stamp_s, cut_frame_num=1,
                    scan_count=1000):
        """process_cut_frame_pcl2 on the device.  Returns [(begin_time_s, offset, count)] per sub-frame."""
        return self._ingest(self.L.lii_ingest_pcl2, data, n_points, lii_pc2_fields(*fields), lidar_type, n_scans,
                            point_filter_num, blind, stamp_s, cut_frame_num, scan_count)

    def ingest_livox(self, data, n_points, fields, n_scans, point_filter_num, blind, stamp_s, cut_frame_num=1, scan_count=1000):
        """process_cut_frame_livox on the device."""
        return self._ingest(self.L.lii_ingest_livox, data, n_points, lii_livox_fields(*fields), 1, n_scans, point_filter_num,
                            blind, stamp_s, cut_frame_num, scan_count)

    def frame_select(self, k: int):
        self._check(self.L.lii_frame_select(self.h, k))

    def ingest_pcl2_begin(self, data, n_points, fields, lidar_type, n_scans, point_filter_num, blind, stamp_s, cut_frame_num=1,
                          scan_count=1000):
        """The overlapped form (ABI 9): the message is put under way and the call returns; `data` (a buffer object) is kept alive here
        until the matching ingest_end."""
        raw = np.frombuffer(data, np.uint8)
        opts = lii_ingest_opts(C.sizeof(lii_ingest_opts), lidar_type, n_scans, point_filter_num, blind, stamp_s, cut_frame_num, scan_count)
        f = lii_pc2_fields(*fields)
        self._check(self.L.lii_ingest_pcl2_begin(self.h, _ptr(raw) if len(raw) else None, n_points, C.byref(f), C.byref(opts)))
        self._ingest_keep = getattr(self, "_ingest_keep", []) + [raw]

    def ingest_livox_begin(self, data, n_points, fields, n_scans, point_filter_num, blind, stamp_s, cut_frame_num=1, scan_count=1000):
        raw = np.frombuffer(data, np.uint8)
        opts = lii_ingest_opts(C.sizeof(lii_ingest_opts), 1, n_scans, point_filter_num, blind, stamp_s, cut_frame_num, scan_count)
        f = lii_livox_fields(*fields)
        self._check(self.L.lii_ingest_livox_begin(self.h, _ptr(raw) if len(raw) else None, n_points, C.byref(f), C.byref(opts)))
        self._ingest_keep = getattr(self, "_ingest_keep", []) + [raw]

    def ingest_end(self):
        """Waits for the oldest message under way; its frames become the ones frame_select serves.  Returns what ingest_pcl2 returns."""
        frames = (lii_frame_info * 64)()
        nf = C.c_int32(0)
        self._check(self.L.lii_ingest_end(self.h, frames, 64, C.byref(nf)))
        if getattr(self, "_ingest_keep", None):
            self._ingest_keep.pop(0)
        self.frame_tail_ms = [frames[k].last_offset_ms for k in range(nf.value)]
        return [(frames[k].begin_time_s, frames[k].offset, frames[k].count) for k in range(nf.value)]

    # ------------------------------------------------------------------ registration
    def iekf_iterate(self, state: State, search: bool, imu_en: bool):
        out = np.zeros(91)
        self._check(self.L.lii_iekf_iterate(self.h, _ptr(state.pod), int(search), int(imu_en), _ptr(out)))
        return out

    def iekf_update(self, state: State, state_prop: State, max_iterations=4, imu_en=False):
        """Runs the whole iterated update in place on `state`; returns the report dict."""
        opts = lii_iekf_opts(int(max_iterations), int(imu_en))
        rep = lii_iekf_report()
        self._check(self.L.lii_iekf_update(self.h, _ptr(state.pod), _ptr(state_prop.pod), C.byref(opts), C.byref(rep)))
        return _report(rep)

    def scan_register(self, state: State, state_prop: State, *, imu_poses=None, cv=False, leaf=0.0, max_iterations=4,
                      imu_en=False, scan_dev=None, scan_sorted=False, map_update=False, next_scan=None, while_waiting=None):
        """Undistortion + voxel grid + iterated update in one library call (one host synchronisation).  scan_dev: a
        device_scan() handle to adopt first (what scan_set_device would do, without the separate call).  scan_sorted: True / 1 - the
        points are in ascending time order; 2 / "sort" - the library sorts them by time on the device first
        (lii_scan_job::scan_sorted; register_imu and register_cv take the same values).  map_update: map_incremental with the final state
        follows inside the call (lii_scan_job::map_update) - do not call map_incremental() for this scan."""
        job, _alive = _scan_job(1 if imu_poses is not None else (2 if cv else 0), imu_poses, leaf, max_iterations, imu_en, scan_dev, scan_sorted,
                                map_update, next_scan, while_waiting)
        rep = lii_iekf_report()
        self._check(self.L.lii_scan_register(self.h, C.byref(job), _ptr(state.pod), _ptr(state_prop.pod), C.byref(rep)))
        return _report(rep)

    # ------------------------------------------------------------------ per-point measurement noise (calcBodyVar, src/laserMapping.cpp:158-181)
    def set_point_noise(self, range_inc=0.02, degree_inc=0.05):
        """lii_point_noise_set, model 1: every fit pass from here on weights a selected point by R_inv_i = 1 / sigma^2_i,
        sigma^2_i = LASER_POINT_COV + the range term along the ray + the bearing term across it (the arguments of calcBodyVar at
        src/laserMapping.cpp:1041: 0.02 m, 0.05 deg) - a standing setting of the handle, off by default."""
        m = lii_point_noise(C.sizeof(lii_point_noise), 1, float(range_inc), float(degree_inc))
        self._check(self.L.lii_point_noise_set(self.h, C.byref(m)))

    def clear_point_noise(self):
        """Back to model 0: R_inv = laser_point_cov_inv for every point (src/laserMapping.cpp:1050)."""
        self._check(self.L.lii_point_noise_set(self.h, None))

    def point_noise(self):
        """dict(model, range_inc, degree_inc) as the handle holds them."""
        m = lii_point_noise(C.sizeof(lii_point_noise), 0, 0.0, 0.0)
        self._check(self.L.lii_point_noise_get(self.h, C.byref(m)))
        return dict(model=int(m.model), range_inc=float(m.range_inc), degree_inc=float(m.degree_inc))

    def point_noise_download(self):
        """(n,) float32: (float)sqrt(R_inv_i) of every point of the down-sampled cloud as the last fit pass left it - 0 where the point
        was not selected - in the device's order (the intensity src/laserMapping.cpp:1051 stores).  LIIError(-5) under model 0 or before
        the first pass."""
        n = C.c_int32(0)
        out = np.zeros(max(self.max_scan_points, 1), np.float32)
        self._check(self.L.lii_point_noise_download(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), len(out), C.byref(n)))
        return out[:n.value].copy()

    # ------------------------------------------------------------------ IMU processing (ImuProcess::Process on the device)
    def set_imu_noise(self, cov_gyr=None, cov_acc=None, cov_bias_gyr=None, cov_bias_acc=None, cov_R_LI=None, cov_T_LI=None,
                      mean_acc_norm=None):
        """The setters of ImuProcess (src/IMU_Processing.hpp:127-159); what is left None keeps the constructor's value
        (lii_imu_noise_defaults).  Scalars are spread over the three axes."""
        nz = lii_imu_noise()
        self._check(self.L.lii_imu_noise_defaults(C.byref(nz)), None)
        for name, v in (("cov_gyr", cov_gyr), ("cov_acc", cov_acc), ("cov_bias_gyr", cov_bias_gyr), ("cov_bias_acc", cov_bias_acc),
                        ("cov_R_LI", cov_R_LI), ("cov_T_LI", cov_T_LI)):
            if v is not None:
                getattr(nz, name)[:] = list(np.broadcast_to(np.asarray(v, np.float64), (3,)))
        if mean_acc_norm is not None:
            nz.mean_acc_norm = float(mean_acc_norm)
        self._check(self.L.lii_imu_set_noise(self.h, C.byref(nz)))

    @property
    def imu_carry(self):
        """dict(last_imu (7,) = t, gyr, acc; acc_s_last, angvel_last, last_lidar_end_time) - the members ImuProcess keeps between scans."""
        c = lii_imu_carry()
        self._check(self.L.lii_imu_get_carry(self.h, C.byref(c)))
        return dict(last_imu=np.r_[c.last_imu.t, c.last_imu.gyr[:], c.last_imu.acc[:]], acc_s_last=np.array(c.acc_s_last[:]),
                    angvel_last=np.array(c.angvel_last[:]), last_lidar_end_time=float(c.last_lidar_end_time))

    @imu_carry.setter
    def imu_carry(self, d):
        c = lii_imu_carry()
        li = np.asarray(d["last_imu"], np.float64).reshape(7)
        c.last_imu.t = float(li[0])
        c.last_imu.gyr[:] = list(li[1:4])
        c.last_imu.acc[:] = list(li[4:7])
        c.acc_s_last[:] = list(np.asarray(d.get("acc_s_last", np.zeros(3)), np.float64))
        c.angvel_last[:] = list(np.asarray(d.get("angvel_last", np.zeros(3)), np.float64))
        c.last_lidar_end_time = float(d.get("last_lidar_end_time", 0.0))
        self._check(self.L.lii_imu_set_carry(self.h, C.byref(c)))

    def propagate_imu(self, imu, pcl_beg_time, pcl_end_time, state: State):
        """The forward part of propagation_and_undist (:292-382).  imu: (n, 7) rows (t, gyr, acc).  Returns (propagated state,
        IMUpose table (K, 22)); `state` is left as it was, the handle's carry is advanced."""
        imu = np.ascontiguousarray(imu, np.float64).reshape(-1, 7)
        out = state.copy()
        poses = pose6d_array(len(imu) + 1)
        k = C.c_int32(0)
        self._check(self.L.lii_imu_propagate(self.h, _ptr(imu) if len(imu) else None, len(imu), float(pcl_beg_time), float(pcl_end_time),
                                             _ptr(out.pod), _ptr(poses), len(poses), C.byref(k)))
        return out, poses[:k.value]

    def propagate_cv(self, dt, cov_gyr_scale, cov_acc_scale, state: State):
        """Forward_propagation_without_imu without its de-skew (:212-244); returns the propagated state."""
        out = state.copy()
        cg = np.ascontiguousarray(np.broadcast_to(np.asarray(cov_gyr_scale, np.float64), (3,)))
        ca = np.ascontiguousarray(np.broadcast_to(np.asarray(cov_acc_scale, np.float64), (3,)))
        self._check(self.L.lii_cv_propagate(self.h, float(dt), _ptr(cg), _ptr(ca), _ptr(out.pod)))
        return out

    def register_imu(self, imu, pcl_beg_time, state: State, *, leaf=0.0, max_iterations=4, imu_en=True, scan_dev=None, scan_sorted=False,
                     map_update=False, next_scan=None, while_waiting=None, imu_poses=None, want_propagated=True):
        """ImuProcess::Process + de-skew + voxel grid + iterated update in one library call (lii_scan_register_imu): `state` in is the
        state after the previous update and is updated in place.  Returns (state, propagated state or None, report dict).  The
        keywords are scan_register's; imu_poses must stay None (the table is formed on the device)."""
        imu = np.ascontiguousarray(imu, np.float64).reshape(-1, 7)
        job, _alive = _scan_job(1, imu_poses, leaf, max_iterations, imu_en, scan_dev, scan_sorted, map_update, next_scan, while_waiting)
        rep = lii_iekf_report()
        prop = State() if want_propagated else None
        self._check(self.L.lii_scan_register_imu(self.h, C.byref(job), _ptr(imu) if len(imu) else None, len(imu), float(pcl_beg_time),
                                                 _ptr(state.pod), _ptr(prop.pod) if prop is not None else None, C.byref(rep)))
        return state, prop, _report(rep)

    def register_cv(self, dt, cov_gyr_scale, cov_acc_scale, state: State, *, leaf=0.0, max_iterations=4, scan_dev=None, scan_sorted=False,
                    map_update=False, while_waiting=None, imu_poses=None, want_propagated=True, undistort=2):
        """Process() with imu_en == false + voxel grid + iterated update in one library call (lii_scan_register_cv): the constant-velocity
        propagation rides in the de-skew launch.  `state` in is the state after the previous update and is updated in place.  Returns
        (state, propagated state or None, report dict).  imu_poses must stay None and undistort 2 (the rules' tests pass others)."""
        cg = None if cov_gyr_scale is None else np.ascontiguousarray(np.broadcast_to(np.asarray(cov_gyr_scale, np.float64), (3,)))
        ca = None if cov_acc_scale is None else np.ascontiguousarray(np.broadcast_to(np.asarray(cov_acc_scale, np.float64), (3,)))
        job, _alive = _scan_job(undistort, imu_poses, leaf, max_iterations, 0, scan_dev, scan_sorted, map_update, None, while_waiting)
        rep = lii_iekf_report()
        prop = State() if want_propagated else None
        self._check(self.L.lii_scan_register_cv(self.h, C.byref(job), float(dt), _ptr(cg) if cg is not None else None,
                                                _ptr(ca) if ca is not None else None, _ptr(state.pod),
                                                _ptr(prop.pod) if prop is not None else None, C.byref(rep)))
        return state, prop, _report(rep)

    # ------------------------------------------------------------------ the registered clouds (publish_frame_world / pcd_save)
    def publish_set(self, clouds=0, to_host=False, save_capacity=0):
        """The standing order (lii_publish_set): clouds = PUB_DENSE | PUB_DOWN | PUB_EFFECT | PUB_BODY (| PUB_INTENSITY: the
        intensities of DENSE / DOWN / BODY beside them); nothing ordered: off."""
        if not clouds and not save_capacity:
            self._check(self.L.lii_publish_set(self.h, None))
            return
        o = lii_publish_opts(C.sizeof(lii_publish_opts), int(clouds), int(bool(to_host)), int(save_capacity))
        self._check(self.L.lii_publish_set(self.h, C.byref(o)))

    def publish_now(self, state: State):
        self._check(self.L.lii_publish_now(self.h, _ptr(state.pod)))

    def publish_fetch(self, cloud, copy=True):
        """One cloud of the last finished registration as an (n, 4) float32 array: a view of the library's pinned buffer (to_host;
        copy=False - valid until the registration after the next one begins) or a copy; without to_host the device buffer is
        downloaded.  Callable from while_waiting of the next call."""
        hp, dp, n = C.c_void_p(), C.c_void_p(), C.c_int32(0)
        self._check(self.L.lii_publish_fetch(self.h, int(cloud), C.byref(hp), C.byref(dp), C.byref(n)))
        if n.value == 0:
            return np.zeros((0, 4), np.float32)
        if hp.value:
            a = np.ctypeslib.as_array(C.cast(hp, C.POINTER(C.c_float)), shape=(n.value, 4))
            return a.copy() if copy else a
        import torch  # (device only: the buffer is read through torch, the project's plumbing)
        return torch.as_tensor(_DeviceFloat4(dp.value, n.value), device="cuda").cpu().numpy().copy()

    def publish_fetch_intensity(self, cloud, copy=True):
        """The intensities of one cloud (PUB_DENSE, PUB_DOWN or PUB_BODY) of the last finished registration as (n,) float32, row for row
        with publish_fetch(cloud); the same lifetime, callable from while_waiting of the next call."""
        hp, dp, n = C.c_void_p(), C.c_void_p(), C.c_int32(0)
        self._check(self.L.lii_publish_fetch_intensity(self.h, int(cloud), C.byref(hp), C.byref(dp), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, np.float32)
        if hp.value:
            a = np.ctypeslib.as_array(C.cast(hp, C.POINTER(C.c_float)), shape=(n.value,))
            return a.copy() if copy else a
        import torch  # (device only: the buffer is read through torch, the project's plumbing)
        return torch.as_tensor(_DeviceFloat(dp.value, n.value), device="cuda").cpu().numpy().copy()

    def publish_saved_intensity(self):
        """The save buffer's intensities as (n,) float32, point for point with publish_saved(); LIIError(-4) as publish_saved."""
        n = C.c_int32(0)
        rc = self.L.lii_publish_saved_intensity(self.h, None, 0, C.byref(n))
        if rc not in (0, -4):
            self._check(rc)
        out = np.zeros(max(n.value, 1), np.float32)
        self._check(self.L.lii_publish_saved_intensity(self.h, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    def publish_saved(self, clear=False):
        """The save buffer (pcl_wait_save) as an (n, 4) float32 array; LIIError(-4) if a scan did not fit since the last clear."""
        n = C.c_int32(0)
        rc = self.L.lii_publish_saved(self.h, None, 0, C.byref(n), 0)
        if rc not in (0, -4):
            self._check(rc)
        out = np.zeros((max(n.value, 1), 4), np.float32)
        self._check(self.L.lii_publish_saved(self.h, _ptr(out), len(out), C.byref(n), int(bool(clear))))
        return out[:n.value]

    # ------------------------------------------------------------------ ... as message bytes (pcl::toROSMsg / PCDWriter::writeBinary)
    def publish_wire_set(self, clouds=0, to_host=False):
        """The second standing order (lii_publish_wire_set): the ordered clouds (PUB_DENSE | PUB_DOWN | PUB_EFFECT | PUB_BODY) as the
        bytes of sensor_msgs/PointCloud2::data, 48-byte pcl::PointXYZINormal records; nothing ordered: off."""
        if not clouds:
            self._check(self.L.lii_publish_wire_set(self.h, None))
            return
        o = lii_wire_opts(C.sizeof(lii_wire_opts), int(clouds), int(bool(to_host)), 0)
        self._check(self.L.lii_publish_wire_set(self.h, C.byref(o)))

    def publish_wire_fetch(self, cloud, copy=True):
        """One cloud of the last finished registration as an (n, 48) uint8 array - msg.data, row for row with publish_fetch(cloud): a
        view of the library's pinned buffer (to_host; copy=False - valid until the registration after the next one begins) or a copy;
        without to_host the device buffer is downloaded.  Callable from while_waiting of the next call."""
        hp, dp, n = C.c_void_p(), C.c_void_p(), C.c_int32(0)
        self._check(self.L.lii_publish_wire_fetch(self.h, int(cloud), C.byref(hp), C.byref(dp), C.byref(n)))
        if n.value == 0:
            return np.zeros((0, 48), np.uint8)
        if hp.value:
            a = np.ctypeslib.as_array(C.cast(hp, C.POINTER(C.c_uint8)), shape=(n.value, 48))
            return a.copy() if copy else a
        import torch  # (device only: the buffer is read through torch, the project's plumbing)
        return torch.as_tensor(_DeviceFloat(dp.value, 12 * n.value), device="cuda").cpu().numpy().view(np.uint8).reshape(n.value, 48).copy()

    def publish_saved_pcd(self, clear=False):
        """The save buffer as the rows of a binary PCD, an (n, 32) uint8 array (x y z normal_x normal_y normal_z intensity curvature),
        repacked on the device; pcd_header(n) + rows.tobytes() is the file.  LIIError(-4) if a scan did not fit since the last clear."""
        n = C.c_int32(0)
        rc = self.L.lii_publish_saved_pcd(self.h, None, 0, C.byref(n), 0)
        if rc not in (0, -4):
            self._check(rc)
        out = np.zeros((max(n.value, 1), 32), np.uint8)
        self._check(self.L.lii_publish_saved_pcd(self.h, _ptr(out), out.nbytes, C.byref(n), int(bool(clear))))
        return out[:n.value]

    @staticmethod
    def wire_layout():
        """lii_publish_wire_layout (host only, no handle): see the module's wire_layout()."""
        return wire_layout()

    @staticmethod
    def pcd_header(n_points):
        """lii_pcd_header (host only, no handle): see the module's pcd_header()."""
        return pcd_header(n_points)

    def neighbors(self, n):
        pts = np.zeros((n, 5, 3), np.float32)
        cnt = np.zeros(n, np.int32)
        sel = np.zeros(n, np.uint8)
        self._check(self.L.lii_neighbors_download(self.h, _ptr(pts), _ptr(cnt), _ptr(sel), n))
        return pts, cnt, sel

    def map_incremental(self, state: State, want_counts: bool = True):
        """want_counts=False: both size pointers NULL - the update is enqueued without a host round trip (predicted list sizes)."""
        if not want_counts:
            self._check(self.L.lii_map_incremental(self.h, _ptr(state.pod), None, None))
            return None
        a, b = C.c_int32(0), C.c_int32(0)
        self._check(self.L.lii_map_incremental(self.h, _ptr(state.pod), C.byref(a), C.byref(b)))
        return a.value, b.value

    # ------------------------------------------------------------------ calibration
    def calib_set_buffers(self, imu22, lidar22):
        imu = np.ascontiguousarray(imu22, np.float64).reshape(-1, 22)
        lid = np.ascontiguousarray(lidar22, np.float64).reshape(-1, 22)
        assert len(imu) == len(lid)
        self._check(self.L.lii_calib_set_buffers(self.h, _ptr(imu), _ptr(lid), len(imu)))

    def calib_eval(self, stage, params):
        dof = {1: 3, 2: 7, 3: 9}[stage]
        p = np.ascontiguousarray(params, np.float64).reshape(-1)
        JtJ, Jtr, cost = np.zeros((dof, dof)), np.zeros(dof), C.c_double(0)
        self._check(self.L.lii_calib_eval(self.h, stage, _ptr(p), _ptr(JtJ), _ptr(Jtr), C.byref(cost)))
        return JtJ, Jtr, cost.value

    def calib_solve_stage(self, stage, result=None):
        res = result if result is not None else lii_calib_result()
        if result is None:
            res.R_LI[:] = list(np.eye(3).reshape(-1))
        self._check(self.L.lii_calib_solve_stage(self.h, stage, C.byref(res)))
        return res

    def li_init_run(self, imu22, lidar22, orig_odom_freq, cut_frame_num):
        """LI_Init::LI_Initialization after downsample_interpolate_IMU; returns (lii_calib_result, time_lag_1, total_lag)."""
        imu = np.ascontiguousarray(imu22, np.float64).reshape(-1, 22)
        lid = np.ascontiguousarray(lidar22, np.float64).reshape(-1, 22)
        res = lii_calib_result()
        l1, tot = C.c_double(0), C.c_double(0)
        self._check(self.L.lii_li_init_run(self.h, _ptr(imu), _ptr(lid), len(imu), int(orig_odom_freq), int(cut_frame_num),
                                           C.byref(res), C.byref(l1), C.byref(tot)))
        return res, l1.value, tot.value

    def zero_phase_filter(self, seqs22):
        """LI_Init::zero_phase_filt on the device: seqs22 (n_seq, n, 22) -> filtered copy."""
        a = np.ascontiguousarray(seqs22, np.float64)
        assert a.ndim == 3 and a.shape[2] == 22
        out = np.zeros_like(a)
        self._check(self.L.lii_zero_phase_filter(self.h, _ptr(a), a.shape[0], a.shape[1], _ptr(out)))
        return out

    def xcorr_lag(self, imu22, lidar22) -> int:
        """LI_Init::xcorr_temporal_init on the device: lag_IMU_wtr_Lidar in samples."""
        imu = np.ascontiguousarray(imu22, np.float64).reshape(-1, 22)
        lid = np.ascontiguousarray(lidar22, np.float64).reshape(-1, 22)
        lag = C.c_int32(0)
        self._check(self.L.lii_xcorr_lag(self.h, _ptr(imu), _ptr(lid), len(imu), C.byref(lag)))
        return lag.value

    def li_init_set_device(self, on: bool):
        self._check(self.L.lii_li_init_set_device(self.h, int(on)))

    def li_init_resident(self, imu22, lidar22, orig_odom_freq, cut_frame_num, interpolate=False, move_start_time=0.0):
        """LI_Init::LI_Initialization resident on the device: one upload, a fixed sequence of launches, one wait.
        interpolate = False: the aligned sequences li_init_run takes; True: every raw IMU state and every LiDAR-odometry state
        (downsample_interpolate_IMU runs first).  Returns (lii_calib_result, lii_li_init_report)."""
        imu = np.ascontiguousarray(imu22, np.float64).reshape(-1, 22)
        lid = np.ascontiguousarray(lidar22, np.float64).reshape(-1, 22)
        job = lii_li_init_job(C.sizeof(lii_li_init_job), int(bool(interpolate)), imu.ctypes.data, len(imu), lid.ctypes.data, len(lid),
                              float(move_start_time), int(orig_odom_freq), int(cut_frame_num))
        res, rep = lii_calib_result(), lii_li_init_report()
        rep.struct_size = C.sizeof(lii_li_init_report)
        self._check(self.L.lii_li_init_resident(self.h, C.byref(job), C.byref(res), C.byref(rep)))
        return res, rep

    def li_init_resident_fetch(self, which):
        """The sequences the last resident run solved on: which = 1 entering stages 1 / 2, which = 2 entering stage 3.
        Returns (imu22, lidar22)."""
        n = C.c_int32(0)
        self._check(self.L.lii_li_init_resident_fetch(self.h, int(which), None, None, 0, C.byref(n)))
        imu, lid = calib_state_array(n.value), calib_state_array(n.value)
        if n.value:
            self._check(self.L.lii_li_init_resident_fetch(self.h, int(which), _ptr(imu), _ptr(lid), n.value, C.byref(n)))
        return imu, lid

    def li_init_windows_records(self, imu22, lidar22, windows, orig_odom_freq, cut_frame_num, interpolate=False):
        """lii_li_init_windows: LI_Initialization on every window of the sequences in one call (one upload, a fixed number of
        launches whatever the number of windows, one wait).  windows: what li_init_prefix_windows / li_init_sliding_windows
        return, or rows (begin, count) - aligned form - or (imu_begin, imu_count, lidar_begin, lidar_count[, move_start_time]).
        Returns the ctypes array of lii_li_init_window_result, one per window."""
        imu = np.ascontiguousarray(imu22, np.float64).reshape(-1, 22)
        lid = np.ascontiguousarray(lidar22, np.float64).reshape(-1, 22)
        win = li_init_window_array(windows)
        job = lii_li_init_job(C.sizeof(lii_li_init_job), int(bool(interpolate)), imu.ctypes.data, len(imu), lid.ctypes.data, len(lid),
                              0.0, int(orig_odom_freq), int(cut_frame_num))
        out = (lii_li_init_window_result * max(len(win), 1))()
        self._check(self.L.lii_li_init_windows(self.h, C.byref(job), win.ctypes.data, len(win), C.addressof(out),
                                               C.sizeof(lii_li_init_window_result)))
        return out

    def li_init_windows(self, imu22, lidar22, windows, orig_odom_freq, cut_frame_num, interpolate=False):
        """li_init_windows_records as a structured array of LI_INIT_WINDOW_DTYPE (a refused window: its status, zeros behind it)."""
        out = self.li_init_windows_records(imu22, lidar22, windows, orig_odom_freq, cut_frame_num, interpolate)
        rec = np.zeros(len(out), LI_INIT_WINDOW_DTYPE)
        for k, q in enumerate(out):
            r = rec[k]
            r["status"] = q.status
            r["R_LI"] = np.array(q.res.R_LI[:]).reshape(3, 3)
            for f in ("T_LI", "gyro_bias", "acc_bias", "grav_L0", "iterations", "final_cost"):
                r[f] = getattr(q.res, f)[:]
            r["time_lag_2"] = q.res.time_lag_2
            r["termination"] = q.rep.termination[:]
            for f in ("time_lag_1", "total_time_lag", "n_aligned", "n_stage12", "n_stage3", "lag_samples"):
                r[f] = getattr(q.rep, f)
        return rec

    def li_init_windows_scratch(self):
        """(bytes of device scratch li_init_windows holds on this handle, allocations its calls have made so far)"""
        b, a = C.c_uint64(0), C.c_int64(0)
        self._check(self.L.lii_li_init_windows_scratch(self.h, C.byref(b), C.byref(a)))
        return b.value, a.value

    def calib_solve_stage_dev(self, stage, result=None):
        """calib_solve_stage with the whole Levenberg-Marquardt in one launch."""
        res = result if result is not None else lii_calib_result()
        if result is None:
            res.R_LI[:] = list(np.eye(3).reshape(-1))
        self._check(self.L.lii_calib_solve_stage_dev(self.h, stage, C.byref(res)))
        return res

    # ------------------------------------------------------------------ multi-GPU
    def comm_unique_id(self) -> bytes:
        buf = (C.c_uint8 * 128)()
        self._check(self.L.lii_comm_unique_id(buf), None)
        return bytes(buf)

    def comm_init(self, n_ranks, rank, uid: bytes, transport="auto"):
        """transport: "auto" (peer-mapped HBM mailbox when all ranks share the node, else the host-memory mailbox, else RCCL),
        "rccl", "mailbox" (HBM, over HIP IPC), "mailbox_host"."""
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._check(self.L.lii_comm_init_ex(self.h, n_ranks, rank, buf, {"auto": 0, "rccl": 1, "mailbox": 2, "mailbox_host": 3}[transport]))

    def comm_set_partition(self, library_partition):
        """True / 1 / "index" (default): every rank hands over the whole scan, the library splits the down-sampled cloud into
        contiguous blocks; 2 / "voxel": ... by voxel - a rank filters and registers the voxels whose key hashes to it (where the
        filter is fused into the de-skew: lii_scan_register; by index elsewhere); False / 0 / "caller": the caller hands every
        rank its own points."""
        mode = {"caller": 0, "index": 1, "voxel": 2}.get(library_partition, library_partition)
        self._check(self.L.lii_comm_set_partition(self.h, int(mode)))

    def comm_transport(self) -> str:
        t = C.c_int32(0)
        self._check(self.L.lii_comm_transport(self.h, C.byref(t)))
        return {0: "none", 1: "rccl", 2: "mailbox", 3: "mailbox_host"}[t.value]

    def comm_describe(self) -> str:
        buf = C.create_string_buffer(512)
        self._check(self.L.lii_comm_describe(self.h, buf, 512))
        return buf.value.decode()

    def comm_rccl_ranks(self) -> int:
        """ncclCommCount of the attached RCCL communicator (0: no RCCL communicator)."""
        n = C.c_int32(0)
        self._check(self.L.lii_comm_rccl_ranks(self.h, C.byref(n)))
        return int(n.value)

    def last_solve_info(self):
        """Passes of the last device-resident update whose 12 x 12 elimination needed the routine with row exchanges."""
        n = C.c_int32(0)
        self._check(self.L.lii_last_solve_info(self.h, C.byref(n)))
        return int(n.value)

    def last_unfinished_queries(self):
        """Queries the most recent search pass left to the fit launch behind it."""
        n = C.c_int32(0)
        self._check(self.L.lii_last_unfinished_queries(self.h, C.byref(n)))
        return int(n.value)

    def selftest_list_exchange(self, add_lists, nodown_lists, form):
        """The list exchange of a sharded job's map update played by ONE handle for len(add_lists) ranks (form "gather": the mailbox
        transport's gather areas, "allgather": the trimmed all-gather layout of the RCCL transport); rank r's lists are (n, 4) float32.
        Returns the joined (add, nodown) lists every played rank ended with."""
        n = len(add_lists)
        assert n == len(nodown_lists) and n >= 1
        na = np.array([len(a) for a in add_lists], np.int32)
        nn = np.array([len(a) for a in nodown_lists], np.int32)
        cat = lambda ls: np.ascontiguousarray(np.concatenate([np.asarray(a, np.float32).reshape(-1, 4) for a in ls] + [np.zeros((1, 4), np.float32)]))
        a, d = cat(add_lists), cat(nodown_lists)
        cap = int(max(na.sum(), nn.sum(), 1))
        oa, od = np.zeros((cap, 4), np.float32), np.zeros((cap, 4), np.float32)
        ona, onn = C.c_int32(0), C.c_int32(0)
        self._check(self.L.lii_selftest_list_exchange(self.h, n, {"gather": 0, "allgather": 1}[form], _ptr(a), _ptr(na), _ptr(d), _ptr(nn),
                                                      _ptr(oa), C.byref(ona), _ptr(od), C.byref(onn), cap))
        return oa[:ona.value].copy(), od[:onn.value].copy()

    def comm_destroy(self):
        self._check(self.L.lii_comm_destroy(self.h))

    def set_profiling(self, enabled: bool):
        """Turns the HIP-event timing of the registration kernels on/off and zeroes the accumulators."""
        self._check(self.L.lii_set_profiling(self.h, int(enabled)))  # 1 = start (zero), 2 = resume, 0 = pause

    def timings(self):
        """[0] sum ms search-pass kernel, [1] sum ms residual-pass kernel, [2] sum ms reduce kernel, [3] host solve ms of
        the last update, [4] total ms of the last update, [5]/[6] launch counts behind [0]/[1]."""
        out = np.zeros(8)
        self._check(self.L.lii_last_timings(self.h, _ptr(out)))
        return out

    def kernel_profile(self):
        """Per-launch brackets of lii_scan_register collected under set_profiling(3): {kind: (total ms, launches)}, scans."""
        kp = lii_kernel_profile()
        kp.struct_size = C.sizeof(lii_kernel_profile)
        self._check(self.L.lii_last_kernel_profile(self.h, C.byref(kp)))
        return {k: (kp.ms[i], kp.launches[i]) for i, k in enumerate(KERNEL_KINDS)}, kp.scans
