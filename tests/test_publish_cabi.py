"""CPU-side checks of the registered-cloud entry points (include/liinit_hip.h: lii_publish_set / _now / _fetch / _saved - what
laserMapping's loop hands out behind the update, src/laserMapping.cpp:1152-1156): exported, declared and mirrored, lii_publish_opts is
16 bytes, NULL handles and bad arguments are refused without touching a device, and the ABI stays where it was (version 9,
lii_scan_job 88 bytes, lii_kernel_profile unchanged: the launch takes the free kind 7)."""
import ctypes as C
import os
import re

import numpy as np

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lii_publish_set", "lii_publish_now", "lii_publish_fetch", "lii_publish_saved")
INVALID = -1


def _header():
    hdr = open(os.path.join(ROOT, "include", "liinit_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_new_symbols_exported_declared_and_mirrored():
    L = C.CDLL(lii.library_path())
    _, code = _header()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in api.EXPORTED_SYMBOLS, name
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in the header"
    for m in ("publish_set", "publish_now", "publish_fetch", "publish_saved"):
        assert hasattr(api.Registrar, m), m


def test_struct_and_abi():
    hdr, code = _header()
    assert C.sizeof(api.lii_publish_opts) == 16
    body = code[code.index("typedef struct lii_publish_opts {"):code.index("} lii_publish_opts;")]
    assert re.findall(r"^\s*u?int32_t\s+([a-z_]+);", body, re.M) == ["struct_size", "clouds", "to_host", "save_capacity"]
    assert [api.lii_publish_opts.clouds.offset, api.lii_publish_opts.to_host.offset, api.lii_publish_opts.save_capacity.offset] == [4, 8, 12]
    for name, bit in (("DENSE", 1), ("DOWN", 2), ("EFFECT", 4), ("BODY", 8)):
        assert re.search(r"LII_PUB_%s\s*=\s*%d\b" % (name, bit), code) and getattr(api, "PUB_" + name) == bit
    assert int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9
    assert lii.load_library().lii_abi_version() == 9
    assert C.sizeof(api.lii_scan_job) == 88
    # the profile struct keeps its size: the launch is attributed to the kind that was free
    assert re.search(r"LII_KP_PUBLISH\s*=\s*7\b", code) and re.search(r"LII_KP_KINDS\s*=\s*8\b", code)
    assert C.sizeof(api.lii_kernel_profile) == 8 + 8 * 8 + 4 * 8 and api.KERNEL_KINDS.index("publish") == 7


def test_null_handle_and_bad_arguments_are_invalid():
    L = lii.load_library()
    o = api.lii_publish_opts(16, api.PUB_DENSE, 0, 0)
    st = lii.State()
    hp, dp, n = C.c_void_p(), C.c_void_p(), C.c_int32(7)
    buf = np.zeros((4, 4), np.float32)
    assert L.lii_publish_set(None, C.byref(o)) == INVALID
    assert L.lii_publish_set(None, None) == INVALID
    for bad in (api.lii_publish_opts(12, 1, 0, 0), api.lii_publish_opts(16, 16, 0, 0), api.lii_publish_opts(16, 1, 2, 0), api.lii_publish_opts(16, 1, 0, -1)):
        assert L.lii_publish_set(None, C.byref(bad)) == INVALID
    assert L.lii_publish_now(None, st.pod.ctypes.data) == INVALID
    assert L.lii_publish_fetch(None, api.PUB_DENSE, C.byref(hp), C.byref(dp), C.byref(n)) == INVALID
    assert L.lii_publish_fetch(None, 3, C.byref(hp), C.byref(dp), C.byref(n)) == INVALID
    assert L.lii_publish_saved(None, buf.ctypes.data, 4, C.byref(n), 0) == INVALID
    assert n.value == 7 and not hp.value and not dp.value  # nothing was written


def test_the_oracles_point_body_to_world_is_the_plain_double_formula():
    """tests/test_gpu_publish.py compares the clouds with the oracle's restatement of pointBodyToWorld (oracle/orc_iekf.hpp:68-74,
    src/laserMapping.cpp:209-220), reached through a one-pass update on a tiny tree.  Here it is held against the formula written out
    in numpy doubles, left to right, rounded to float once: the same bits."""
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    st = O.state_init()
    v = O.StateView(st)
    from harness import synth
    v.rot_end[:] = synth.rot_zyx(0.3, -0.2, 1.1)
    v.pos_end[:] = [3.1, -2.7, 0.9]
    v.offset_R_L_I[:] = synth.rot_zyx(0.01, 0.02, -0.03)
    v.offset_T_L_I[:] = [0.04, -0.02, 0.11]
    pts = (rng.normal(size=(777, 4)) * 9).astype(np.float32)
    tree = O.Tree("oracle")
    tree.build(rng.normal(size=(32, 3)).astype(np.float32))
    w = tree.iekf_update(pts, st, st, max_iterations=1)["world"]
    b = pts[:, :3].astype(np.float64)
    RLI, TLI, R, p = v.offset_R_L_I, v.offset_T_L_I, v.rot_end, v.pos_end
    imu = [RLI[r, 0] * b[:, 0] + RLI[r, 1] * b[:, 1] + RLI[r, 2] * b[:, 2] + TLI[r] for r in range(3)]
    ref = np.stack([R[r, 0] * imu[0] + R[r, 1] * imu[1] + R[r, 2] * imu[2] + p[r] for r in range(3)], 1).astype(np.float32)
    assert np.array_equal(w.view(np.uint32), ref.view(np.uint32))
