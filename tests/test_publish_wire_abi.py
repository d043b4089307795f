"""The registered clouds as message bytes, host side (no GPU): lii_publish_wire_set / _wire_fetch / _wire_layout, lii_publish_saved_pcd,
lii_pcd_header - the symbols, the structs, the record layout held against an independently written numpy dtype, and the PCD header
text held against the text of PCDWriter::generateHeader for pcl::PointXYZINormal (restated from knowledge of PCL: include/liinit_hip.h
says so)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, CAPACITY = -1, -4
NEW = ("lii_publish_wire_set", "lii_publish_wire_fetch", "lii_publish_wire_layout", "lii_publish_saved_pcd", "lii_pcd_header")

# pcl::PointXYZINormal as pcl::toROSMsg describes it: twelve little-endian 32-bit words, the eight named ones at these offsets
RECORD = np.dtype(dict(names=["x", "y", "z", "normal_x", "normal_y", "normal_z", "intensity", "curvature"],
                       formats=["<f4"] * 8, offsets=[0, 4, 8, 16, 20, 24, 32, 36], itemsize=48))
PCD_ROW = np.dtype([(n, "<f4") for n in RECORD.names])

HEADER = ("# .PCD v0.7 - Point Cloud Data file format\n"
          "VERSION 0.7\n"
          "FIELDS x y z normal_x normal_y normal_z intensity curvature\n"
          "SIZE 4 4 4 4 4 4 4 4\n"
          "TYPE F F F F F F F F\n"
          "COUNT 1 1 1 1 1 1 1 1\n"
          "WIDTH {n}\n"
          "HEIGHT 1\n"
          "VIEWPOINT 0 0 0 1 0 0 0\n"
          "POINTS {n}\n"
          "DATA binary\n")


def test_symbols_exported_and_mirrored():
    L = C.CDLL(lii.library_path())
    hdr = open(os.path.join(ROOT, "include", "liinit_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in api.EXPORTED_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    for method in ("publish_wire_set", "publish_wire_fetch", "publish_saved_pcd", "wire_layout", "pcd_header"):
        assert callable(getattr(lii.Registrar, method)), method


def _c_sizeof(struct):
    """sizeof of a struct of include/liinit_hip.h, from its text: int32_t / uint32_t 4, char[n] n, nested structs by name."""
    hdr = open(os.path.join(ROOT, "include", "liinit_hip.h")).read()
    body = hdr[hdr.index("typedef struct %s {" % struct):hdr.index("} %s;" % struct)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = 0
    for typ, _, dim in re.findall(r"^\s*([a-z0-9_]+)\s+([a-z_0-9]+)(?:\[(\d+)\])?;", body, re.M):
        one = {"int32_t": 4, "uint32_t": 4, "char": 1}.get(typ) or _c_sizeof(typ)
        size += one * int(dim or 1)
    return size


def test_struct_sizes():
    assert C.sizeof(api.lii_wire_opts) == _c_sizeof("lii_wire_opts") == 16
    assert C.sizeof(api.lii_wire_field) == _c_sizeof("lii_wire_field") == 32
    assert C.sizeof(api.lii_wire_layout) == _c_sizeof("lii_wire_layout") == 16 + 8 * 32
    # the library agrees: it refuses any other struct_size
    L = lii.load_library()
    lay = api.lii_wire_layout(struct_size=C.sizeof(api.lii_wire_layout))
    assert L.lii_publish_wire_layout(C.byref(lay)) == 0
    lay.struct_size -= 4
    assert L.lii_publish_wire_layout(C.byref(lay)) == INVALID
    assert L.lii_publish_wire_layout(None) == INVALID
    # the existing order's struct and the ABI number are where they were
    assert C.sizeof(api.lii_publish_opts) == 16 and L.lii_abi_version() == 9


def test_null_handle_is_invalid():
    L = lii.load_library()
    o = api.lii_wire_opts(C.sizeof(api.lii_wire_opts), 1, 0, 0)
    hp, dp, n = C.c_void_p(), C.c_void_p(), C.c_int32(0)
    assert L.lii_publish_wire_set(None, C.byref(o)) == INVALID
    assert L.lii_publish_wire_set(None, None) == INVALID
    assert L.lii_publish_wire_fetch(None, 1, C.byref(hp), C.byref(dp), C.byref(n)) == INVALID
    assert L.lii_publish_saved_pcd(None, None, 0, C.byref(n), 0) == INVALID


def test_layout_equals_the_numpy_dtype():
    lay = lii.wire_layout()
    assert lay == lii.Registrar.wire_layout()
    assert lay["point_step"] == RECORD.itemsize == 48 and lay["pcd_row_bytes"] == PCD_ROW.itemsize == 32
    assert [f[0] for f in lay["fields"]] == list(RECORD.names)
    for name, offset, datatype, count, pcd_offset in lay["fields"]:
        assert offset == RECORD.fields[name][1] and RECORD.fields[name][0] == np.dtype("<f4")
        assert pcd_offset == PCD_ROW.fields[name][1]
        assert datatype == 7 and count == 1  # sensor_msgs/PointField::FLOAT32
    # ... and a dtype BUILT from the answer is the independently written one: twelve words, eight of them named
    built = np.dtype(dict(names=[f[0] for f in lay["fields"]], formats=["<f4"] * 8, offsets=[f[1] for f in lay["fields"]], itemsize=lay["point_step"]))
    assert built == RECORD and built.itemsize // 4 == 12
    one = np.zeros(1, built)
    one["intensity"], one["curvature"] = 2.0, 3.0
    words = one.view("<f4")
    assert words[8] == 2.0 and words[9] == 3.0 and words.shape == (12,)


def _parse(text):
    """FIELDS, SIZE and POINTS of a PCD header"""
    out = {}
    for line in text.splitlines():
        key, _, rest = line.partition(" ")
        if key in ("FIELDS", "SIZE", "POINTS"):
            out[key] = rest.split()
    return out


@pytest.mark.parametrize("n", [0, 1, 1_234_567])
def test_pcd_header(n):
    L = lii.load_library()
    text = lii.pcd_header(n)
    assert text == lii.Registrar.pcd_header(n) == HEADER.format(n=n).encode()
    got = _parse(text.decode())
    assert got["FIELDS"] == list(PCD_ROW.names) and got["SIZE"] == ["4"] * 8 and got["POINTS"] == [str(n)]
    assert sum(int(s) for s in got["SIZE"]) == PCD_ROW.itemsize
    # length only; a capacity too small; the exact capacity (no terminator written behind it); a negative count
    ln = C.c_int32(0)
    assert L.lii_pcd_header(n, None, 0, C.byref(ln)) == 0 and ln.value == len(text)
    small = C.create_string_buffer(len(text) - 1)
    ln = C.c_int32(0)
    assert L.lii_pcd_header(n, small, len(small), C.byref(ln)) == CAPACITY and ln.value == len(text)
    exact = C.create_string_buffer(b"\xAA" * (len(text) + 1), len(text) + 1)
    assert L.lii_pcd_header(n, exact, len(text), C.byref(ln)) == 0 and exact.raw[:len(text)] == text and exact.raw[len(text)] == 0xAA
    assert L.lii_pcd_header(-1, None, 0, C.byref(ln)) == INVALID
    assert L.lii_pcd_header(n, None, 0, None) == INVALID
