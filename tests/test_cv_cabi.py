"""CPU-side checks of the LO-phase additions to include/liinit_hip.h: lii_scan_register_cv and lii_map_build_from_scan are exported,
declared and mirrored, refuse a NULL handle without touching a device, and leave the ABI where it was (version 9, lii_scan_job 88 bytes)."""
import ctypes as C
import os
import re

import numpy as np

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lii_scan_register_cv", "lii_map_build_from_scan")


def test_new_symbols_exported_declared_and_mirrored():
    L = C.CDLL(lii.library_path())
    hdr = open(os.path.join(ROOT, "include", "liinit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in api.EXPORTED_SYMBOLS, name
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in the header"
    assert hasattr(api.Registrar, "register_cv") and hasattr(api.Registrar, "map_build_from_scan")


def test_abi_is_unchanged():
    hdr = open(os.path.join(ROOT, "include", "liinit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9
    assert lii.load_library().lii_abi_version() == 9
    assert C.sizeof(api.lii_scan_job) == 88
    assert re.search(r"LII_KP_KINDS\s*=\s*8\b", code)


def test_null_handle_is_invalid():
    L = lii.load_library()
    rep, job, n = api.lii_iekf_report(), api.lii_scan_job(), C.c_int32(7)
    job.struct_size, job.undistort = C.sizeof(api.lii_scan_job), 2
    job.opts = api.lii_iekf_opts(4, 0)
    st = lii.State()
    three = np.ones(3)
    INVALID = -1
    assert L.lii_scan_register_cv(None, C.byref(job), 0.1, three.ctypes.data, three.ctypes.data, st.pod.ctypes.data, None, C.byref(rep)) == INVALID
    assert L.lii_map_build_from_scan(None, st.pod.ctypes.data, C.byref(n)) == INVALID
