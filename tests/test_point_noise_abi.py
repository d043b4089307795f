"""The per-point noise model at the boundary (no GPU): the three entry points are declared in include/liinit_hip.h, exported by
libliinit_hip.so and mirrored in api.EXPORTED_SYMBOLS with the declared arguments; lii_point_noise has the header's layout; nothing existing
callers compiled against has moved - LII_ABI_VERSION stays 9; the header names the reference lines, the z = 0 defect and the closed form."""
import ctypes
import os
import re

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"lii_point_noise_set": 2, "lii_point_noise_get": 2, "lii_point_noise_download": 4}


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
    for method in ("set_point_noise", "clear_point_noise", "point_noise", "point_noise_download"):
        assert callable(getattr(lii.Registrar, method, None)), method


def test_struct_layout_and_abi_version():
    hdr = _header()
    assert int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9
    assert lii.load_library().lii_abi_version() == 9
    body = re.search(r"typedef struct lii_point_noise \{(.*?)\} lii_point_noise;", _code(), flags=re.S).group(1)
    fields = [(t, n) for t, n in re.findall(r"(uint32_t|int32_t|double)\s+(\w+)\s*;", body)]
    assert fields == [("uint32_t", "struct_size"), ("int32_t", "model"), ("double", "range_inc"), ("double", "degree_inc")]
    ctype = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(api.lii_point_noise._fields_)
    assert ctypes.sizeof(api.lii_point_noise) == 24
    assert api.lii_point_noise.range_inc.offset == 8 and api.lii_point_noise.degree_inc.offset == 16
    assert ctypes.sizeof(api.lii_scan_job) == 88 and ctypes.sizeof(api.lii_config) == 48


def test_header_names_the_reference_lines():
    hdr = _header()
    at = hdr.index("per-point measurement noise from range and bearing")
    text = hdr[at:hdr.index("int lii_point_noise_download", at)]
    for cite in ("src/laserMapping.cpp:1039-1042", ":158-181", ":1050", ":1051", ":170-171", ":625-636", "0.017453293", "z = 0", "CLOSED FORM",
                 "sr2 u^2 / r^2 + s2 |A|^2"):
        assert cite in text, cite
    for name in NEW:
        assert name in text, f"the header comment does not describe {name}"


def test_null_handle_is_refused_without_a_device():
    L = lii.load_library()
    m = api.lii_point_noise(ctypes.sizeof(api.lii_point_noise), 1, 0.02, 0.05)
    n = ctypes.c_int32(0)
    assert L.lii_point_noise_set(None, ctypes.byref(m)) == -1 and L.lii_point_noise_set(None, None) == -1
    assert L.lii_point_noise_get(None, ctypes.byref(m)) == -1
    assert L.lii_point_noise_download(None, None, 0, ctypes.byref(n)) == -1
