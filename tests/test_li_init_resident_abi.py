"""The resident LI-Init at the boundary (no GPU): lii_li_init_resident, lii_li_init_resident_fetch and lii_calib_solve_stage_dev are
declared in include/liinit_hip.h, exported by libliinit_hip.so and mirrored in api.EXPORTED_SYMBOLS with ctypes structs of the header's
layout; LII_ABI_VERSION stays 9 and lii_calib_result keeps its 216 bytes; what the host refuses before anything is enqueued is refused
without a handle."""
import ctypes
import os
import re

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lii_li_init_resident", "lii_li_init_resident_fetch", "lii_calib_solve_stage_dev"]
LII_ERR_INVALID = -1


def _header():
    return open(os.path.join(ROOT, "include", "liinit_hip.h")).read()


def _offsets(struct):
    return [(f[0], getattr(struct, f[0]).offset) for f in struct._fields_]


def test_new_symbols_declared_exported_and_mirrored():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(lii_[a-z0-9_]+)\s*\(", code))
    L = ctypes.CDLL(lii.library_path())
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/liinit_hip.h"
        assert hasattr(L, name), f"{name} is not exported by libliinit_hip.so"
        assert name in api.EXPORTED_SYMBOLS, f"{name} is not mirrored in api.EXPORTED_SYMBOLS"
    for m in ("li_init_resident", "li_init_resident_fetch", "calib_solve_stage_dev"):
        assert callable(getattr(lii.Registrar, m, None)), m


def test_layouts():
    hdr = _header()
    assert int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9
    assert lii.load_library().lii_abi_version() == 9
    # LP64: the pointers are 8 bytes and 8-byte aligned, the doubles likewise
    assert ctypes.sizeof(api.lii_li_init_job) == 56
    assert _offsets(api.lii_li_init_job) == [("struct_size", 0), ("interpolate", 4), ("imu", 8), ("n_imu", 16), ("lidar", 24),
                                             ("n_lidar", 32), ("move_start_time", 40), ("orig_odom_freq", 48), ("cut_frame_num", 52)]
    assert re.search(r"typedef struct lii_li_init_job \{[^}]*uint32_t struct_size;[^}]*int32_t interpolate;[^}]*const lii_calib_state\* imu;"
                     r"[^}]*int32_t n_imu;[^}]*const lii_calib_state\* lidar;[^}]*int32_t n_lidar;[^}]*double move_start_time;"
                     r"[^}]*int32_t orig_odom_freq, cut_frame_num;[^}]*\} lii_li_init_job;", hdr)
    assert ctypes.sizeof(api.lii_li_init_report) == 40 + 16 + 3 * 24 * 8
    assert _offsets(api.lii_li_init_report) == [("struct_size", 0), ("n_aligned", 4), ("n_stage12", 8), ("n_stage3", 12), ("lag_samples", 16),
                                                ("launches", 20), ("host_waits", 24), ("termination", 28), ("time_lag_1", 40),
                                                ("total_time_lag", 48), ("params", 56)]
    assert re.search(r"typedef struct lii_li_init_report \{[^}]*uint32_t struct_size;[^}]*int32_t n_aligned, n_stage12, n_stage3;"
                     r"[^}]*int32_t lag_samples;[^}]*int32_t launches, host_waits;[^}]*int32_t termination\[3\];"
                     r"[^}]*double time_lag_1, total_time_lag;[^}]*double params\[3\]\[24\];[^}]*\} lii_li_init_report;", hdr)
    assert ctypes.sizeof(api.lii_calib_result) == 216  # untouched
    assert ctypes.sizeof(api.lii_scan_job) == 88


def _job(imu, lid, n_imu, n_lidar, interpolate=0, freq=10, cut=5, size=None):
    return api.lii_li_init_job(ctypes.sizeof(api.lii_li_init_job) if size is None else size, interpolate,
                               ctypes.addressof(imu) if imu is not None else None, n_imu,
                               ctypes.addressof(lid) if lid is not None else None, n_lidar, 0.0, freq, cut)


def test_host_side_refusals_without_a_handle():
    """Every refusal the host makes before anything is enqueued.  Without a GPU there is no handle, and a NULL handle is refused with
    the same code: what this shows is that each of these calls returns LII_ERR_INVALID and dereferences nothing;
    tests/test_gpu_li_init_resident.py repeats the argument errors on a live handle."""
    L = lii.load_library()
    buf = (ctypes.c_double * (22 * 256))()
    out = api.lii_calib_result()
    rep = api.lii_li_init_report(ctypes.sizeof(api.lii_li_init_report))
    good = _job(buf, buf, 256, 256)
    assert L.lii_li_init_resident(None, ctypes.byref(good), ctypes.byref(out), ctypes.byref(rep)) == LII_ERR_INVALID
    assert L.lii_li_init_resident(None, None, ctypes.byref(out), None) == LII_ERR_INVALID
    assert L.lii_li_init_resident(None, ctypes.byref(good), None, None) == LII_ERR_INVALID
    bad = [_job(buf, buf, 256, 256, size=8),                  # struct_size
           _job(buf, buf, 256, 256, interpolate=2),           # interpolate other than 0 / 1
           _job(buf, buf, 256, 256, interpolate=-1),
           _job(None, buf, 256, 256), _job(buf, None, 256, 256),   # NULL sequences
           _job(buf, buf, 199, 199),                          # aligned form: n < 200
           _job(buf, buf, 256, 255),                          # aligned form: n_imu != n_lidar
           _job(buf, buf, 5, 200, interpolate=1),             # raw form: n_imu < 6
           _job(buf, buf, 256, 0, interpolate=1),             # raw form: n_lidar < 1
           _job(buf, buf, 256, 256, freq=0), _job(buf, buf, 256, 256, cut=0)]
    for j in bad:
        assert L.lii_li_init_resident(None, ctypes.byref(j), ctypes.byref(out), None) == LII_ERR_INVALID
    bad_rep = api.lii_li_init_report(4)
    assert L.lii_li_init_resident(None, ctypes.byref(good), ctypes.byref(out), ctypes.byref(bad_rep)) == LII_ERR_INVALID
    n = ctypes.c_int32(0)
    assert L.lii_li_init_resident_fetch(None, 1, None, None, 0, ctypes.byref(n)) == LII_ERR_INVALID
    assert L.lii_li_init_resident_fetch(None, 2, None, None, 0, None) == LII_ERR_INVALID
    assert L.lii_calib_solve_stage_dev(None, 1, ctypes.byref(out)) == LII_ERR_INVALID
    assert L.lii_calib_solve_stage_dev(None, 1, None) == LII_ERR_INVALID
