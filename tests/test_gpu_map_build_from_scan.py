"""lii_map_build_from_scan - the first scan seeds the map (src/laserMapping.cpp:921-929) without leaving the device - against the way
the replay host took before: lii_scan_download(1), pointBodyToWorld (:209-220) in numpy fp64 cast to float32, lii_map_build.

Case A of tests/golden/imu/reference_cv_process.npz goes through lii_undistort_cv and lii_downsample(0.1) on two handles.  The two maps
hold the same number of points and, both sets sorted, every coordinate agrees within 1 float ulp: both sides form the fp64 result of
R (R_LI p + T_LI) + t in the same order and round it once, so only that final rounding can differ (numpy's matrix products may contract
or reassociate a sum).  A lii_scan_register_cv against each map finds the same number of effective points."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
LEAF = 0.1


def _ulp_diff(a, b):  # tests/test_gpu_scan_ops.py
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def _registrar():
    import lidar_imu_init_amd as lii
    return lii.Registrar(max_scan_points=20_000, max_map_points=100_000, filter_size_map=0.15)


def _state():
    """An LO-phase state with an extrinsic that is not the identity, so that both halves of pointBodyToWorld show."""
    import lidar_imu_init_amd as lii
    import make_cv_process_fixture as M
    from harness import synth
    st = lii.State(M.load("A")["out_state"])
    st.offset_R_L_I[:] = synth.rot_zyx(0.02, -0.03, 0.5)
    st.offset_T_L_I[:] = [0.05, -0.03, 0.10]
    return st


def _prepare(reg, pts, st):
    reg.scan_upload(pts)
    reg.undistort_cv(st.bias_g, st.vel_end, st.rot_end)
    return reg.downsample(LEAF)


def _sorted_rows(x):
    return x[np.lexsort((x[:, 2], x[:, 1], x[:, 0]))]


def test_map_from_scan_equals_the_host_built_map():
    import lidar_imu_init_amd as lii
    import make_cv_process_fixture as M
    c = M.load("A")
    st = _state()
    # ---- on the device
    reg_a = _registrar()
    _prepare(reg_a, c["pts"], st)
    n_a = reg_a.map_build_from_scan(st)
    map_a = reg_a.map_download()
    # ---- the replay host's way
    reg_b = _registrar()
    _prepare(reg_b, c["pts"], st)
    body = reg_b.scan_download(1)[:, :3].astype(np.float64)
    world = ((body @ st.offset_R_L_I.T + st.offset_T_L_I) @ st.rot_end.T + st.pos_end).astype(np.float32)
    reg_b.map_build(world)
    map_b = reg_b.map_download()
    print(f"map from the scan: {n_a} points ({len(map_a)} downloaded); host-built map: {len(map_b)} points")
    assert n_a == len(map_a) == len(map_b) == len(world) and n_a > 1000
    ulp = _ulp_diff(_sorted_rows(map_a), _sorted_rows(map_b))
    print(f"sorted sets: max {int(ulp.max())} ulp, coordinates that differ: {int((ulp > 0).sum())} of {ulp.size}")
    assert ulp.max() <= 1
    # ---- a registration against each map
    reps = []
    for reg in (reg_a, reg_b):
        reg.scan_upload(c["pts"])
        _, _, rep = reg.register_cv(c["dt"], c["cov_gyr_scale"], c["cov_acc_scale"], lii.State(c["state"]), leaf=LEAF, max_iterations=5, scan_sorted=True)
        reps.append(rep)
        reg.close()
    print("registered against the two maps:", [(r["iterations"], r["effect_num"]) for r in reps])
    assert reps[0]["effect_num"] == reps[1]["effect_num"] > 100


def test_rules_of_lii_map_build_from_scan():
    import lidar_imu_init_amd as lii
    import make_cv_process_fixture as M
    c = M.load("A")
    st = _state()
    reg = _registrar()
    with pytest.raises(lii.LIIError) as e:  # a fresh handle: no down-sampled cloud
        reg.map_build_from_scan(st)
    assert e.value.code == -5  # LII_ERR_STATE
    # five points: `if (feats_down_size > 5)` - nothing is built, LII_OK
    reg.scan_upload(c["pts"][:5])
    assert reg.downsample_skip() == 5
    assert reg.map_build_from_scan(st) == 0
    assert reg.map_size() == 0
    # six are a map
    reg.scan_upload(c["pts"][:6])
    assert reg.downsample_skip() == 6
    assert reg.map_build_from_scan(st) == 6
    assert reg.map_size() == 6
    reg.close()
    # beyond max_map_points
    small = lii.Registrar(max_scan_points=20_000, max_map_points=1000, filter_size_map=0.15)
    small.scan_upload(c["pts"])
    small.downsample_skip()
    with pytest.raises(lii.LIIError) as e:
        small.map_build_from_scan(st)
    assert e.value.code == -4  # LII_ERR_CAPACITY
    small.close()
