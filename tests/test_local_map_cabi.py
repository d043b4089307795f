"""The moving local map at the boundary, without a device: the symbols of lii_local_map_* in the header, the library and the Python
mirror; the layouts of the two structs; harness/fov_harness.py - the numpy restatement of lasermap_fov_segment
(src/laserMapping.cpp:260-305) the GPU tests hold the library to - against values derived by hand; the parameter route; and what
can be refused without a handle: NULL arguments only.  The checks of the VALUES (cube_len <= 3 det_range and the rest) need a handle, and a
handle needs a device: tests/test_gpu_local_map.py::test_refusals makes them."""
import ctypes as C
import os
import re

import numpy as np

import lidar_imu_init_amd as lii
from harness import fov_harness as F
from lidar_imu_init_amd import api, params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lii_local_map_set", "lii_local_map_get", "lii_local_map_segment", "lii_params_local_map")
INVALID = -1


def _header():
    return open(os.path.join(ROOT, "include", "liinit_hip.h")).read()


def test_symbols_in_header_library_and_mirror():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    L = C.CDLL(lii.library_path())
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), n
        assert hasattr(L, n), n
        assert n in api.EXPORTED_SYMBOLS, n
    for m in ("local_map_set", "local_map_get", "local_map_segment"):
        assert callable(getattr(api.Registrar, m))
    assert lii.load_library().lii_abi_version() == 9 == int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert C.sizeof(api.lii_scan_job) == 88  # the switch is handle state: the job is as it was


def _c_fields(name):
    hdr = _header()
    body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"^\s*([a-z0-9_]+)\s+([a-z_0-9]+)(?:\[(\d+)\])?;", body, re.M)


def test_struct_layouts_match_header():
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "float": C.c_float}
    for name, mirror in (("lii_local_map_opts", api.lii_local_map_opts), ("lii_local_map_info", api.lii_local_map_info)):
        want = [(f, ctype[t] * int(n) if n else ctype[t]) for t, f, n in _c_fields(name)]
        got = [(f, t) for f, t in mirror._fields_]
        assert [f for f, _ in got] == [f for f, _ in want], name
        assert all(C.sizeof(a[1]) == C.sizeof(b[1]) for a, b in zip(got, want)), name
        ref = type("ref_" + name, (C.Structure,), {"_fields_": want})
        assert C.sizeof(mirror) == C.sizeof(ref)
    assert C.sizeof(api.lii_local_map_opts) == 24
    assert C.sizeof(api.lii_local_map_info) == 128  # 116 bytes of 4-byte fields, 4 of padding, the 8-byte total
    assert api.lii_local_map_info.deleted_total.offset == 120


def test_restatement_against_hand_derived_values():
    """cube_len 40, det_range 10: thr = 1.5 * 10 = 15; mov_dist = max((40 - 30) * 0.5 * 0.9, 10 * 0.5) = max(4.5, 5) = 5."""
    thr, mov = F.constants(40.0, 10.0)
    assert thr.dtype == np.float32 and mov.dtype == np.float32
    assert thr == np.float32(15.0) and mov == np.float32(5.0)
    cube = F.LocalMapCube(40.0, 10.0)
    assert len(cube.segment([0.0, 0.0, 0.0])) == 0 and cube.initialized
    assert np.array_equal(cube.cube, np.array([-20, -20, -20, 20, 20, 20], np.float32))
    # |x| < 5: the nearer face is more than 15 away, nothing moves
    for x in (0.5, -4.999, 4.999, 3.0):
        assert len(cube.segment([x, 0.0, 0.0])) == 0
        assert np.array_equal(cube.cube, np.array([-20, -20, -20, 20, 20, 20], np.float32)) and cube.moves == 0
    # x = 5 exactly: 20 - 5 = 15 <= 15 on the HIGH side (the low side, 25 away, is tested first and fails).  The cube moves up by 5 and
    # the slab it leaves behind goes: a copy of the old cube with max[0] = old.min[0] + 5 = -15
    boxes = cube.segment([5.0, 0.0, 0.0])
    assert boxes.dtype == np.float32 and np.array_equal(boxes, np.array([[-20, -20, -20, -15, 20, 20]], np.float32))
    assert np.array_equal(cube.cube, np.array([-15, -20, -20, 25, 20, 20], np.float32)) and cube.moves == 1
    # the LOW side, from a fresh cube: x = -5, 15 from the low face.  The cube moves down and min[0] = old.max[0] - 5 = 15
    low = F.LocalMapCube(40.0, 10.0)
    low.segment([0.0, 0.0, 0.0])
    boxes = low.segment([-5.0, 0.0, 0.0])
    assert np.array_equal(boxes, np.array([[15, -20, -20, 20, 20, 20]], np.float32))
    assert np.array_equal(low.cube, np.array([-25, -20, -20, 15, 20, 20], np.float32))
    # two axes in one call: x high, y low - boxes in axis order, both cut from the OLD cube
    two = F.LocalMapCube(40.0, 10.0)
    two.segment([0.0, 0.0, 0.0])
    boxes = two.segment([6.0, -7.0, 1.0])
    assert np.array_equal(boxes, np.array([[-20, -20, -20, -15, 20, 20], [-20, 15, -20, 20, 20, 20]], np.float32))
    assert np.array_equal(two.cube, np.array([-15, -25, -20, 25, 15, 20], np.float32)) and two.moves == 1
    # the delete: min <= p < max - the lower face goes, the upper face stays
    pts = np.array([[-20, 0, 0], [-15, 0, 0], [-15.000001, 0, 0], [0, 0, 0], [-17, 20, 0], [-17, 19.5, 0]], np.float32)
    dead = F.in_boxes(pts, np.array([[-20, -20, -20, -15, 20, 20]], np.float32))
    assert dead.tolist() == [True, False, True, False, False, True]
    assert len(F.delete_boxes(pts, np.zeros((0, 6), np.float32))) == len(pts)


def test_avia_parameters_reach_the_options():
    """launch/avia.launch: cube_side_length 2000; config/avia.yaml: mapping/det_range 450 -> thr 675, mov_dist (2000 - 1350) * 0.45 = 292.5."""
    p = params.Params(launch=os.path.join(ROOT, "harness", "launch", "avia.launch"))
    o = p.local_map()
    assert o.struct_size == C.sizeof(api.lii_local_map_opts) and o.enabled == 1
    assert o.cube_len == 2000.0 and o.det_range == 450.0
    thr, mov = F.constants(o.cube_len, o.det_range)
    assert thr == np.float32(675.0) and mov == np.float32(292.5)


def test_null_arguments_are_refused_without_a_handle():
    L = lii.load_library()
    p = params.Params()
    o = api.lii_local_map_opts()
    assert L.lii_params_local_map(None, C.byref(o)) == INVALID
    assert L.lii_params_local_map(C.byref(p.pod), None) == INVALID
    bad = params.lii_params()
    C.memmove(C.byref(bad), C.byref(p.pod), C.sizeof(bad))
    bad.struct_size = 12
    assert L.lii_params_local_map(C.byref(bad), C.byref(o)) == INVALID
    # the reference's own defaults, 200 / 300, come through as they are: it is lii_local_map_set that judges them (cube_len <= 3 det_range)
    o = p.local_map()
    assert (o.cube_len, o.det_range, o.enabled) == (200.0, 300.0, 1)
    assert not o.cube_len > 3.0 * o.det_range
    info = api.lii_local_map_info()
    pos = (C.c_double * 3)(0.0, 0.0, 0.0)
    assert L.lii_local_map_set(None, C.byref(o)) == INVALID
    assert L.lii_local_map_get(None, C.byref(info)) == INVALID
    assert L.lii_local_map_segment(None, pos, C.byref(info)) == INVALID
    assert L.lii_local_map_segment(None, None, None) == INVALID
