"""CPU-side checks of the IMU processing section of include/liinit_hip.h (ImuProcess::Process on the device): the new symbols are
exported and mirrored, the structs have the header's sizes, lii_imu_noise_defaults gives the constructor's values
(src/IMU_Processing.hpp:97-102) and every handle-taking call refuses a NULL handle without touching a device."""
import ctypes as C
import os
import re

import numpy as np

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lii_imu_noise_defaults", "lii_imu_set_noise", "lii_imu_set_carry", "lii_imu_get_carry", "lii_imu_propagate", "lii_cv_propagate",
       "lii_scan_register_imu")


def test_new_symbols_exported_and_mirrored():
    L = C.CDLL(lii.library_path())
    hdr = open(os.path.join(ROOT, "include", "liinit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in api.EXPORTED_SYMBOLS, name
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in the header"
    assert re.search(r"LII_KP_PROPAGATE\s*=\s*6\b", code) and re.search(r"LII_KP_KINDS\s*=\s*8\b", code)
    assert api.KERNEL_KINDS.index("propagate") == 6
    assert int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9 and C.sizeof(api.lii_scan_job) == 88


def test_struct_sizes():
    assert C.sizeof(api.lii_imu_sample) == 56
    assert C.sizeof(api.lii_imu_carry) == 56 + 56
    assert C.sizeof(api.lii_imu_noise) == 8 + 19 * 8
    assert api.lii_imu_carry.acc_s_last.offset == 56 and api.lii_imu_carry.last_lidar_end_time.offset == 104
    assert api.lii_imu_noise.cov_gyr.offset == 8 and api.lii_imu_noise.mean_acc_norm.offset == 8 + 18 * 8


def test_noise_defaults_are_the_constructors():
    L = lii.load_library()
    nz = api.lii_imu_noise()
    assert L.lii_imu_noise_defaults(C.byref(nz)) == 0
    assert nz.struct_size == C.sizeof(api.lii_imu_noise)
    assert list(nz.cov_gyr) == [0.1] * 3 and list(nz.cov_acc) == [0.1] * 3
    assert list(nz.cov_R_LI) == [0.00001] * 3 and list(nz.cov_T_LI) == [0.0001] * 3
    assert list(nz.cov_bias_gyr) == [0.0001] * 3 and list(nz.cov_bias_acc) == [0.0001] * 3
    # IMU_mean_acc_norm has no default in the constructor: main() installs the parameter
    from lidar_imu_init_amd import params as P
    prm = P.lii_params()
    assert L.lii_params_defaults(C.byref(prm)) == 0
    assert nz.mean_acc_norm == prm.mean_acc_norm > 0
    assert L.lii_imu_noise_defaults(None) == -1


def test_null_handle_is_invalid():
    L = lii.load_library()
    nz, carry, rep, job, k = api.lii_imu_noise(), api.lii_imu_carry(), api.lii_iekf_report(), api.lii_scan_job(), C.c_int32(0)
    assert L.lii_imu_noise_defaults(C.byref(nz)) == 0
    job.struct_size, job.undistort = C.sizeof(api.lii_scan_job), 1
    job.opts = api.lii_iekf_opts(4, 1)
    imu = np.zeros((2, 7))
    st = lii.State()
    poses = np.zeros((3, 22))
    three = np.ones(3)
    INVALID = -1
    assert L.lii_imu_set_noise(None, C.byref(nz)) == INVALID
    assert L.lii_imu_set_carry(None, C.byref(carry)) == INVALID
    assert L.lii_imu_get_carry(None, C.byref(carry)) == INVALID
    assert L.lii_imu_propagate(None, imu.ctypes.data, 2, 0.0, 0.1, st.pod.ctypes.data, poses.ctypes.data, 3, C.byref(k)) == INVALID
    assert L.lii_cv_propagate(None, 0.1, three.ctypes.data, three.ctypes.data, st.pod.ctypes.data) == INVALID
    assert L.lii_scan_register_imu(None, C.byref(job), imu.ctypes.data, 2, 0.0, st.pod.ctypes.data, None, C.byref(rep)) == INVALID
