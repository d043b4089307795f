"""lii_map_surface / lii_map_surface_dev / lii_map_crispness / lii_sym3_eigen at the boundary (no GPU): the four entry points are declared
in include/liinit_hip.h, exported by libliinit_hip.so and mirrored in api.EXPORTED_SYMBOLS; struct lii_surface (88 bytes) and struct
lii_map_crispness (56 bytes) have the header's layout in ctypes and numpy; LII_ABI_VERSION stays 9; NULL handles and the bad arguments of
the handle-free solver are refused without a device."""
import ctypes
import os
import re

import numpy as np

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lii_map_surface", "lii_map_surface_dev", "lii_map_crispness", "lii_sym3_eigen"]
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
    for m in ("map_surface", "map_surface_dev", "map_crispness"):
        assert callable(getattr(lii.Registrar, m, None)), m
    assert callable(lii.sym3_eigen) and callable(api.sym3_eigen)


def test_layouts():
    hdr = _header()
    assert int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9
    assert lii.load_library().lii_abi_version() == 9
    assert ctypes.sizeof(api.lii_surface) == 88
    assert _offsets(api.lii_surface) == [("count", 0), ("valid", 4), ("mean", 8), ("eig", 32), ("normal", 56), ("curvature", 80)]
    assert re.search(r"struct lii_surface \{[^}]*int32_t count;[^}]*int32_t valid;[^}]*double\s+mean\[3\];[^}]*double\s+eig\[3\];"
                     r"[^}]*double\s+normal\[3\];[^}]*double\s+curvature;[^}]*\};", hdr)
    d = api.SURFACE_DTYPE
    assert d.itemsize == 88 and [(n, d.fields[n][1]) for n in d.names] == _offsets(api.lii_surface)
    assert lii.SURFACE_DTYPE is d
    assert ctypes.sizeof(api.lii_map_crispness) == 56
    assert _offsets(api.lii_map_crispness) == [("n_selected", 0), ("n_used", 8), ("n_sparse", 16), ("n_degenerate", 24), ("mme", 32), ("mpv", 40),
                                               ("mean_count", 48)]
    assert re.search(r"struct lii_map_crispness \{[^}]*int64_t n_selected, n_used, n_sparse[^}]*n_degenerate[^}]*double\s+mme;[^}]*double\s+mpv;"
                     r"[^}]*double\s+mean_count;[^}]*\};", hdr)
    # the formula a test mirrors and the selection hash are written where a caller reads them
    assert "C_ab = s2_ab / n - mean_rel_a * mean_rel_b" in hdr
    assert "0x9E3779B1u" in hdr and "0x85EBCA77u" in hdr and "0xC2B2AE3Du" in hdr and "h ^= h >> 15" in hdr


def test_null_and_invalid_arguments_are_refused_without_a_device():
    L = lii.load_library()
    q = np.zeros((4, 3), np.float32)
    out = np.full(4, 7, np.uint8).repeat(88)
    sent = out.copy()
    assert L.lii_map_surface(None, q.ctypes.data, 4, 12, 1.0, None, out.ctypes.data) == LII_ERR_INVALID
    assert L.lii_map_surface_dev(None, q.ctypes.data, 4, 12, 1.0, None, out.ctypes.data) == LII_ERR_INVALID
    assert L.lii_map_surface(None, None, 0, 12, 1.0, None, None) == LII_ERR_INVALID
    assert np.array_equal(out, sent)
    cr = api.lii_map_crispness(7, 7, 7, 7, 7.0, 7.0, 7.0)
    assert L.lii_map_crispness(None, 0.25, 5, 1, ctypes.byref(cr)) == LII_ERR_INVALID
    assert L.lii_map_crispness(None, 0.25, 5, 1, None) == LII_ERR_INVALID
    assert (cr.n_selected, cr.n_used, cr.mme, cr.mean_count) == (7, 7, 7.0, 7.0)
    # the handle-free solver: NULL arguments and non-finite entries
    m, eig, vec = np.array([2.0, 0.5, 0.0, 3.0, 0.25, 1.0]), np.full(3, 7.0), np.full(9, 7.0)
    assert L.lii_sym3_eigen(None, eig.ctypes.data, vec.ctypes.data) == LII_ERR_INVALID
    assert L.lii_sym3_eigen(m.ctypes.data, None, vec.ctypes.data) == LII_ERR_INVALID
    assert L.lii_sym3_eigen(m.ctypes.data, eig.ctypes.data, None) == LII_ERR_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(6):
            mb = m.copy()
            mb[k] = bad
            assert L.lii_sym3_eigen(mb.ctypes.data, eig.ctypes.data, vec.ctypes.data) == LII_ERR_INVALID
    assert (eig == 7.0).all() and (vec == 7.0).all()
    assert L.lii_sym3_eigen(m.ctypes.data, eig.ctypes.data, vec.ctypes.data) == 0
    assert np.all(np.diff(eig) >= 0) and abs(eig.sum() - 6.0) < 1e-14
    try:
        lii.sym3_eigen([np.nan, 0, 0, 1, 0, 1])
    except lii.LIIError as e:
        assert e.code == LII_ERR_INVALID
    else:
        raise AssertionError("a NaN entry was accepted")
