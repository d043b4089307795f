"""Map points keep their intensity, at the boundary (no GPU): the new entry points are declared in include/liinit_hip.h, exported by
libliinit_hip.so and mirrored in api.EXPORTED_SYMBOLS with the declared number of arguments; nothing existing callers compiled against has
moved - LII_ABI_VERSION stays 9, lii_scan_job stays 88 bytes; the header names the reference lines the entry points mirror."""
import ctypes
import os
import re

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry point -> number of arguments (the 3-float sibling's, plus intensity_offset for the two inputs)
NEW = {"lii_map_build_xyzi": 5, "lii_map_add_points_xyzi": 7, "lii_map_download_xyzi": 4, "lii_map_nearest_xyzi": 9,
       "lii_map_nearest_xyzi_dev": 9, "lii_map_radius_xyzi": 11, "lii_map_radius_xyzi_dev": 11, "lii_map_box_search_xyzi": 6,
       "lii_map_removed_acquire_xyzi": 5, "lii_map_pcd": 4, "lii_map_intensity_set": 2, "lii_map_intensity_get": 2}
SIBLING = {"lii_map_download_xyzi": "lii_map_download", "lii_map_nearest_xyzi": "lii_map_nearest", "lii_map_nearest_xyzi_dev": "lii_map_nearest_dev",
           "lii_map_radius_xyzi": "lii_map_radius", "lii_map_radius_xyzi_dev": "lii_map_radius_dev", "lii_map_box_search_xyzi": "lii_map_box_search",
           "lii_map_removed_acquire_xyzi": "lii_map_removed_acquire"}


def _header():
    return open(os.path.join(ROOT, "include", "liinit_hip.h")).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)


def _declared_args(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", _code(), flags=re.S)
    assert m, f"{name} is not declared in include/liinit_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_declared_exported_and_mirrored():
    declared = set(re.findall(r"\b(lii_[a-z0-9_]+)\s*\(", _code()))
    L = ctypes.CDLL(lii.library_path())
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/liinit_hip.h"
        assert hasattr(L, name), f"{name} is not exported by libliinit_hip.so"
        assert name in api.EXPORTED_SYMBOLS, f"{name} is not mirrored in api.EXPORTED_SYMBOLS"
    # ... and the three sets are the same set, new entry points included
    assert sorted(declared) == sorted(api.EXPORTED_SYMBOLS)
    assert not [n for n in declared if not hasattr(L, n)]
    methods = ["map_build_xyzi", "map_add_points_xyzi", "map_download_xyzi", "map_nearest_xyzi", "map_nearest_xyzi_dev", "map_radius_xyzi",
               "map_radius_xyzi_dev", "map_box_search_xyzi", "map_removed_acquire_xyzi", "map_pcd", "map_intensity_set", "map_intensity_get"]
    assert all(callable(getattr(lii.Registrar, m, None)) for m in methods)


def test_argument_counts():
    for name, n_args in NEW.items():
        assert len(_declared_args(name)) == n_args, (name, _declared_args(name))
        restype, argtypes = api._DECLS[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args, name
    for name, sib in SIBLING.items():  # an output is its sibling with wider rows: the same argument types
        assert api._DECLS[name][1] == api._DECLS[sib][1], (name, sib)
    assert api._DECLS["lii_map_build_xyzi"][1] == api._DECLS["lii_map_build"][1] + [ctypes.c_int32]
    a = api._DECLS["lii_map_add_points"][1]
    assert api._DECLS["lii_map_add_points_xyzi"][1] == a[:4] + [ctypes.c_int32] + a[4:]
    assert api._DECLS["lii_map_pcd"][1][2] is ctypes.c_int64  # capacity in bytes, as lii_publish_saved_pcd


def test_nothing_existing_moved():
    hdr = _header()
    assert int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9
    assert lii.load_library().lii_abi_version() == 9
    assert ctypes.sizeof(api.lii_scan_job) == 88
    assert ctypes.sizeof(api.lii_config) == 48 and ctypes.sizeof(api.lii_map_removed_info) == 32
    for name in SIBLING.values():
        assert name in api.EXPORTED_SYMBOLS


def test_header_names_the_reference_lines():
    hdr = _header()
    at = hdr.index("map points keep their intensity")
    text = hdr[at:hdr.index("int lii_map_build_xyzi", at)]
    for cite in ["src/laserMapping.cpp:516-559", ":219", "ikd_Tree.cpp:381-456", ":349-379", ":970-998", ":522-534", "src/laserMapping.cpp:921-931",
                 "include/common_lib.h:37"]:
        assert cite in text, cite
    for name in NEW:
        assert name in text, f"the header comment does not describe {name}"
    # the history's records: the fourth float is no longer "unspecified"
    view = hdr[hdr.index("Order: unspecified - the buffer is a multiset"):hdr.index("Overflow: the delete always completes")]
    assert "intensity" in view and "fourth" in view and "float unspecified" not in view


def test_null_handle_is_refused_without_a_device():
    L = lii.load_library()
    n, t = ctypes.c_int32(0), ctypes.c_int64(0)
    assert L.lii_map_build_xyzi(None, None, 0, 16, 12) == -1
    assert L.lii_map_add_points_xyzi(None, None, 0, 16, 12, 1, ctypes.byref(n)) == -1
    assert L.lii_map_download_xyzi(None, None, 0, ctypes.byref(n)) == -1
    assert L.lii_map_nearest_xyzi(None, None, 0, 12, 5, 5.0, None, None, ctypes.byref(n)) == -1
    assert L.lii_map_nearest_xyzi_dev(None, None, 0, 12, 5, 5.0, None, None, ctypes.byref(n)) == -1
    assert L.lii_map_radius_xyzi(None, None, 0, 12, 1.0, 0, ctypes.byref(t), None, None, 0, ctypes.byref(t)) == -1
    assert L.lii_map_radius_xyzi_dev(None, None, 0, 12, 1.0, 0, ctypes.byref(t), None, None, 0, ctypes.byref(t)) == -1
    assert L.lii_map_box_search_xyzi(None, None, 0, None, 0, ctypes.byref(n)) == -1
    assert L.lii_map_removed_acquire_xyzi(None, None, 0, ctypes.byref(n), 0) == -1
    assert L.lii_map_pcd(None, None, 0, ctypes.byref(n)) == -1
    assert L.lii_map_intensity_set(None, 1) == -1 and L.lii_map_intensity_get(None, ctypes.byref(n)) == -1
