"""lidar_imu_init_amd — MI355X-native (gfx950) hot path of LI-Init behind a C-ABI.

The product is `lib/libliinit_hip.so` (hand-written HIP kernels + C++ host, see include/liinit_hip.h).
This package is the thin Python mirror used by tests, bench.py and harnesses: ctypes bindings only —
no compute happens in Python and nothing here falls back to a CPU implementation.
"""
from .api import (LI_INIT_WINDOW_DTYPE, LI_INIT_WINDOW_IN_DTYPE, SURFACE_DTYPE, LIIError, Registrar, State, calib_state_array,  # noqa: F401
                  li_init_prefix_windows, li_init_sliding_windows, li_init_spread, li_init_window_array, library_path, load_library,
                  pcd_header, pose6d_array, pose_grid, rank_poses, sym3_eigen, wire_layout)

__all__ = ["LIIError", "Registrar", "State", "load_library", "library_path", "calib_state_array", "pose6d_array", "wire_layout", "pcd_header",
           "pose_grid", "rank_poses", "LI_INIT_WINDOW_DTYPE", "LI_INIT_WINDOW_IN_DTYPE", "li_init_window_array", "li_init_prefix_windows",
           "li_init_sliding_windows", "li_init_spread", "SURFACE_DTYPE", "sym3_eigen"]
