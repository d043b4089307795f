"""lii_pose_refine / lii_pose_refine_dev at the boundary (no GPU): both are declared in include/liinit_hip.h beside lii_pose_score,
exported by libliinit_hip.so and mirrored in api.EXPORTED_SYMBOLS with the declared arguments; struct lii_pose_refined has the header's
408-byte layout and api.POSE_REFINED_DTYPE mirrors it; nothing existing callers compiled against has moved - LII_ABI_VERSION stays 9."""
import ctypes
import os
import re

import numpy as np

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api
from pose_refine_cases import RECORD_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"lii_pose_refine": 8, "lii_pose_refine_dev": 8}


def _header():
    return open(os.path.join(ROOT, "include", "liinit_hip.h")).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)


def test_declared_exported_and_mirrored():
    declared = set(re.findall(r"\b(lii_[a-z0-9_]+)\s*\(", _code()))
    L = ctypes.CDLL(lii.library_path())
    for name, n_args in NEW.items():
        assert name in declared, f"{name} is not declared in include/liinit_hip.h"
        assert hasattr(L, name), f"{name} is not exported by libliinit_hip.so"
        assert name in api.EXPORTED_SYMBOLS, f"{name} is not mirrored in api.EXPORTED_SYMBOLS"
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", _code(), flags=re.S)
        assert len(m.group(1).split(",")) == n_args, name
        restype, argtypes = api._DECLS[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args, name
    assert sorted(declared) == sorted(api.EXPORTED_SYMBOLS)
    for method in ("pose_refine", "pose_refine_dev", "relocalize"):
        assert callable(getattr(lii.Registrar, method, None)), method
    # beside lii_pose_score, in front of the edits by point and box
    code = _code()
    assert code.index("int lii_pose_score_dev") < code.index("struct lii_pose_refined") < code.index("int lii_pose_refine") < code.index("int lii_map_delete_points")


def test_struct_layout_and_abi_version():
    hdr = _header()
    assert int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9
    assert lii.load_library().lii_abi_version() == 9
    body = re.search(r"struct lii_pose_refined \{(.*?)\};", _code(), flags=re.S).group(1)
    fields = [(t, n, int(k) if k else 1) for t, n, k in re.findall(r"(int32_t|double)\s+(\w+)\s*(?:\[(\d+)\])?\s*;", body)]
    assert fields == [("double", "pose", 12), ("double", "cov", 36), ("double", "total_residual", 1), ("int32_t", "effect_num", 1),
                      ("int32_t", "iterations", 1), ("int32_t", "searches", 1), ("int32_t", "flags", 1)]
    size = {"double": 8, "int32_t": 4}
    assert sum(size[t] * k for t, _, k in fields) == 408
    for dt in (api.POSE_REFINED_DTYPE, RECORD_DTYPE):
        assert dt.itemsize == 408 and list(dt.names) == [n for _, n, _ in fields]
        at = 0
        for t, n, k in fields:
            assert dt.fields[n][1] == at and dt.fields[n][0].base == np.dtype("<f8" if t == "double" else "<i4"), n
            at += size[t] * k
    flags = dict(re.findall(r"(LII_REFINE_\w+)\s*=\s*(\d+)", _code()))
    assert flags == {"LII_REFINE_CONVERGED": "1", "LII_REFINE_BAD_POSE": "2"}
    assert (api.LII_REFINE_CONVERGED, api.LII_REFINE_BAD_POSE) == (1, 2)


def test_header_says_what_the_call_is():
    hdr = _header()
    at = hdr.index("candidate poses refined against the map in one call")
    text = hdr[at:hdr.index("int lii_pose_refine_dev", at)]
    for cite in ("src/laserMapping.cpp:957-1134", ":1063-1066", ":981-984", ":1081-1087", ":1093-1133", "lii_iekf_update(imu_en = 0)", "other 18 states",
                 "2^22", "LII_ERR_STATE", "LII_ERR_INVALID", "positive definite", "DETERMINISTIC", "lii_point_noise_set"):
        assert cite in text, cite


def test_null_handle_is_refused_without_a_device():
    L = lii.load_library()
    base = lii.State()
    P = np.zeros((1, 12))
    out = np.zeros(1, RECORD_DTYPE)
    for f in (L.lii_pose_refine, L.lii_pose_refine_dev):
        assert f(None, base.pod.ctypes.data, None, P.ctypes.data, 1, 4, 2, out.ctypes.data) == -1
    assert not out.view(np.uint8).any()
