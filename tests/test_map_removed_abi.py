"""The history of removed points at the boundary (no GPU): the four lii_map_removed_* symbols are declared in include/liinit_hip.h,
exported by libliinit_hip.so and mirrored in api.EXPORTED_SYMBOLS; lii_map_removed_info is 32 bytes; nothing existing callers compiled
against has moved (LII_ABI_VERSION 9, lii_local_map_opts 24, lii_local_map_info 128, lii_scan_job 88 bytes); NULL arguments are refused
without a handle.  And the device tests' own expectation - numpy's min <= p < max - is held to the UNMODIFIED reference tree where
oracle/_ref is built: what its Delete_Point_Boxes leaves, joined with the brute-force removed points, is the map before."""
import ctypes
import os
import re

import numpy as np
import pytest

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api
import map_removed_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lii_map_removed_set", "lii_map_removed_get", "lii_map_removed_acquire", "lii_map_removed_view"]


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
    for m in ("map_removed_set", "map_removed_get", "map_removed_acquire", "map_removed_view", "global_map"):
        assert callable(getattr(lii.Registrar, m, None)), m


def test_layouts():
    hdr = _header()
    assert int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9
    assert lii.load_library().lii_abi_version() == 9
    assert ctypes.sizeof(api.lii_map_removed_info) == 32
    assert [(f[0], getattr(api.lii_map_removed_info, f[0]).offset) for f in api.lii_map_removed_info._fields_] == [
        ("struct_size", 0), ("capacity", 4), ("held", 8), ("reserved", 12), ("collected_total", 16), ("lost_total", 24)]
    assert re.search(r"typedef struct lii_map_removed_info \{[^}]*uint32_t struct_size;[^}]*int32_t capacity;[^}]*int32_t held;[^}]*int32_t reserved;"
                     r"[^}]*int64_t collected_total;[^}]*int64_t lost_total;[^}]*\} lii_map_removed_info;", hdr)
    assert ctypes.sizeof(api.lii_local_map_opts) == 24
    assert ctypes.sizeof(api.lii_local_map_info) == 128
    assert ctypes.sizeof(api.lii_scan_job) == 88


def test_null_arguments_are_refused_without_a_handle():
    L = lii.load_library()
    n = ctypes.c_int32(0)
    p = ctypes.c_void_p()
    info = api.lii_map_removed_info(ctypes.sizeof(api.lii_map_removed_info))
    assert L.lii_map_removed_set(None, 16) == -1
    assert L.lii_map_removed_get(None, ctypes.byref(info)) == -1
    assert L.lii_map_removed_acquire(None, None, 0, ctypes.byref(n), 0) == -1
    assert L.lii_map_removed_view(None, ctypes.byref(p), ctypes.byref(n)) == -1


@pytest.mark.parametrize("case", MC.CASES)
def test_expectation_against_the_reference_tree(oracle, small_world, case):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref is not built here (the reference tree is a checker of machines that hold the reference)")
    pts, cases = MC.world(small_world)
    boxes, dead = cases[case]
    tree = oracle.Tree("ref")
    tree.build(pts)
    n = tree.delete_boxes(boxes)
    after = tree.flatten()
    tree.close()
    print(f"{case}: {len(boxes)} boxes, brute force removes {int(dead.sum())} of {len(pts)}, the reference tree {n}")
    assert n == int(dead.sum())
    assert MC.same_multiset(after, pts[~dead])
    assert MC.same_multiset(np.concatenate([after, pts[dead]]), pts)  # before - after = removed
