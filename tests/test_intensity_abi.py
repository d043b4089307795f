"""The intensity channel at the boundary (no GPU): the new symbols are declared in include/liinit_hip.h, exported by libliinit_hip.so and
mirrored in api.EXPORTED_SYMBOLS; nothing that existing callers compiled against has moved - LII_ABI_VERSION stays 9, lii_publish_opts
stays 16 bytes with LII_PUB_INTENSITY as one more bit of `clouds`, lii_scan_job stays 88 bytes."""
import ctypes
import os
import re

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lii_scan_intensity_upload", "lii_scan_intensity_set_device", "lii_ingest_set_intensity", "lii_scan_intensity_download",
       "lii_publish_fetch_intensity", "lii_publish_saved_intensity"]


def _header():
    return open(os.path.join(ROOT, "include", "liinit_hip.h")).read()


def test_new_symbols_declared_exported_and_mirrored():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(lii_[a-z0-9_]+)\s*\(", code))
    L = ctypes.CDLL(lii.library_path())
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/liinit_hip.h"
        assert hasattr(L, name), f"{name} is not exported by libliinit_hip.so"
        assert name in api.EXPORTED_SYMBOLS, f"{name} is not mirrored in api.EXPORTED_SYMBOLS"
    reg_methods = ["scan_intensity_upload", "scan_intensity_set_device", "ingest_set_intensity", "scan_intensity_download",
                   "publish_fetch_intensity", "publish_saved_intensity"]
    assert all(callable(getattr(lii.Registrar, m, None)) for m in reg_methods)


def test_nothing_existing_moved():
    hdr = _header()
    assert int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9
    assert lii.load_library().lii_abi_version() == 9
    assert ctypes.sizeof(api.lii_publish_opts) == 16
    assert ctypes.sizeof(api.lii_scan_job) == 88
    assert [f[0] for f in api.lii_publish_opts._fields_] == ["struct_size", "clouds", "to_host", "save_capacity"]
    assert re.search(r"LII_PUB_INTENSITY\s*=\s*16\b", hdr) and api.PUB_INTENSITY == 16
    assert (api.PUB_DENSE, api.PUB_DOWN, api.PUB_EFFECT, api.PUB_BODY) == (1, 2, 4, 8)


def test_null_handle_is_refused_without_a_device():
    L = lii.load_library()
    n = ctypes.c_int32(0)
    assert L.lii_scan_intensity_upload(None, None, 0, 4, 0) == -1
    assert L.lii_scan_intensity_set_device(None, None, 0) == -1
    assert L.lii_ingest_set_intensity(None, 1) == -1
    assert L.lii_scan_intensity_download(None, 0, None, 0, ctypes.byref(n)) == -1
    assert L.lii_publish_fetch_intensity(None, 1, None, None, ctypes.byref(n)) == -1
    assert L.lii_publish_saved_intensity(None, None, 0, ctypes.byref(n)) == -1
