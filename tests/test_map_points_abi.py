"""Map edits and queries by point and box at the boundary (no GPU): lii_map_delete_points, lii_map_delete_points_dev, lii_map_range and
lii_map_box_search are declared in include/liinit_hip.h, exported by libliinit_hip.so and mirrored in api.EXPORTED_SYMBOLS with ctypes
signatures; the header cites the reference lines they mirror and says why Add_Point_Boxes is not offered; LII_ABI_VERSION stays 9; NULL
arguments are refused without a handle.  And the device tests' model of a point delete on a duplicate-free map - one-ulp boxes
[p, nextafter(p, +inf)) through Delete_Point_Boxes - is held to the UNMODIFIED reference tree where oracle/_ref is built."""
import ctypes
import os
import re

import numpy as np
import pytest

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api
import map_removed_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lii_map_delete_points", "lii_map_delete_points_dev", "lii_map_range", "lii_map_box_search"]


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
        restype, argtypes = api._DECLS[name]
        assert restype is ctypes.c_int and argtypes[0] is ctypes.c_void_p
    assert len(api._DECLS["lii_map_delete_points"][1]) == 5
    assert len(api._DECLS["lii_map_delete_points_dev"][1]) == 4
    assert len(api._DECLS["lii_map_range"][1]) == 2
    assert len(api._DECLS["lii_map_box_search"][1]) == 6
    for m in ("map_delete_points", "map_delete_points_dev", "map_range", "map_box_search"):
        assert callable(getattr(lii.Registrar, m, None)), m


def test_header_cites_the_reference_and_the_abi_stays():
    hdr = _header()
    assert int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9
    assert lii.load_library().lii_abi_version() == 9
    at = hdr.index("lii_map_delete_points <-")
    block = hdr[at:hdr.index("int lii_map_box_search", at)]
    for cite in ("ikd_Tree.cpp:479", "ikd_Tree.cpp:90", "ikd_Tree.cpp:970", ":672-719", ":1269-1271"):
        assert cite in block, cite
    assert "Add_Point_Boxes" in block and "unspecified" in block.lower()
    # the history section names the point delete among what it collects
    hist = hdr[hdr.index("the history of what leaves the local map"):hdr.index("typedef struct lii_map_removed_info")]
    assert "lii_map_delete_points" in hist


def test_null_arguments_are_refused_without_a_handle():
    L = lii.load_library()
    n = ctypes.c_int32(0)
    r = (ctypes.c_float * 6)()
    assert L.lii_map_delete_points(None, None, 0, 12, ctypes.byref(n)) == -1
    assert L.lii_map_delete_points_dev(None, None, 0, 12) == -1
    assert L.lii_map_range(None, r) == -1
    assert L.lii_map_box_search(None, None, 0, None, 0, ctypes.byref(n)) == -1


def test_one_ulp_boxes_model_a_point_delete_in_the_reference_tree(oracle):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref is not built here (the reference tree is a checker of machines that hold the reference)")
    rng = np.random.default_rng(5)
    pts = np.unique(rng.uniform(-10, 10, (3000, 3)).astype(np.float32), axis=0)
    pick = rng.choice(len(pts), 257, replace=False)
    p = pts[pick]
    assert (p != 0).all()
    boxes = np.concatenate([p, np.nextafter(p, np.float32(np.inf))], axis=1).astype(np.float32)
    tree = oracle.Tree("ref")
    tree.build(pts)
    n = tree.delete_boxes(boxes)
    after = tree.flatten()
    tree.close()
    keep = np.ones(len(pts), bool)
    keep[pick] = False
    assert n == 257
    assert MC.same_multiset(after, pts[keep])
