"""The ROS-free C++ host (harness/li_init_replay.cpp) with lii_replay_set_publish: the standing order is placed once, every scan's
clouds are fetched where the reference publishes them (src/laserMapping.cpp:1152-1156) and the save buffer is flushed every
pcd_save_interval scans (:603-612) - on the Ouster stream of tests/test_gpu_replay_device_lo.py, against the same host with publishing
off: publishing changes nothing else, so the final status and every log row are the same BITS; the last scan's dense cloud is
pointBodyToWorld (:209-220, the oracle's restatement) of that scan at the logged state, bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
DENSE, DOWN, EFFECT, BODY = 1, 2, 4, 8
SAVE_INTERVAL = 7


def _cloud(d, rp, which):
    n = C.c_int32(0)
    assert d.lii_replay_cloud(rp, which, None, 0, C.byref(n)) == 0
    out = np.zeros((max(n.value, 1), 4), np.float32)
    assert d.lii_replay_cloud(rp, which, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)) == 0
    return out[:n.value]


def _run(d, T, launch, msgs, imu, fields, msg_period, publish):
    from lidar_imu_init_amd import api
    T._bind(d)
    d.lii_replay_set_device_imu.argtypes = [C.c_void_p, C.c_int32]
    d.lii_replay_set_publish.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    d.lii_replay_cloud.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    d.lii_replay_handle.restype = C.c_void_p
    d.lii_replay_handle.argtypes = [C.c_void_p]
    t_imu, gyro, accel = imu
    cfg = T.ReplayConfig(C.sizeof(T.ReplayConfig), 0, 40_000, 600_000, launch.encode(), None, None, 0, 0)
    rp = C.c_void_p()
    assert d.lii_replay_create(C.byref(cfg), C.byref(rp)) == 0
    assert d.lii_replay_set_device_imu(rp, 1) == 0
    assert d.lii_replay_set_publish(None, DENSE, 0) == -1 and d.lii_replay_set_publish(rp, 16, 0) == -1
    if publish:
        assert d.lii_replay_set_publish(rp, DENSE | DOWN | EFFECT | BODY, SAVE_INTERVAL) == 0
    k_imu = 0
    rows_seen, flushes_checked, prev_dense, prev_rows = 0, 0, None, -1
    for stamp, raw, n in msgs:
        while k_imu < len(t_imu) and t_imu[k_imu] <= stamp + msg_period:
            g, a = np.ascontiguousarray(gyro[k_imu]), np.ascontiguousarray(accel[k_imu])
            assert d.lii_replay_imu(rp, float(t_imu[k_imu]), T._dp(g), T._dp(a)) == 0
            k_imu += 1
        assert d.lii_replay_pcl2(rp, stamp, raw.ctypes.data_as(C.c_void_p), n, C.byref(fields)) == 0
        rc = d.lii_replay_spin(rp)
        assert rc >= 0, d.lii_replay_last_error(rp)
        if publish:  # a flush falls on every SAVE_INTERVAL-th registered scan: where that scan is the last of this spin, the flush ends with its dense cloud
            rows = C.c_int32(0)
            assert d.lii_replay_log(rp, None, 0, C.byref(rows)) == 0
            if rows.value > rows_seen and rows.value % SAVE_INTERVAL == 0:
                flush, dense = _cloud(d, rp, 0), _cloud(d, rp, DENSE)
                assert len(dense) > 0 and len(flush) >= SAVE_INTERVAL * len(dense) // 2
                assert np.array_equal(flush[-len(dense):].view(np.uint32), dense.view(np.uint32)), rows.value
                # ... and holds SAVE_INTERVAL scans, the one before it included (kept from the previous spin when it was that spin's last)
                if prev_dense is not None and prev_rows == rows.value - 1:
                    assert np.array_equal(flush[-len(dense) - len(prev_dense):-len(dense)].view(np.uint32), prev_dense.view(np.uint32)), rows.value
                flushes_checked += 1
            if rows.value > rows_seen:
                prev_dense, prev_rows = _cloud(d, rp, DENSE), rows.value
            rows_seen = rows.value
    n_rows = C.c_int32(0)
    assert d.lii_replay_log(rp, None, 0, C.byref(n_rows)) == 0
    log = np.zeros((n_rows.value, 40))
    assert d.lii_replay_log(rp, log.ctypes.data_as(C.c_void_p), n_rows.value, C.byref(n_rows)) == 0
    ST = T._status_type()
    status = ST()
    status.struct_size = C.sizeof(ST)
    assert d.lii_replay_get_status(rp, C.byref(status)) == 0
    clouds = None
    if publish:
        clouds = {c: _cloud(d, rp, c) for c in (DENSE, DOWN, EFFECT, BODY, 0)}
        L = api.load_library()
        h = d.lii_replay_handle(rp)
        cnt = C.c_int32(0)
        scan = np.zeros((40_000, 4), np.float32)
        assert L.lii_scan_download(h, 0, scan.ctypes.data, len(scan), C.byref(cnt)) == 0
        clouds["scan"] = scan[:cnt.value].copy()
        clouds["flushes_checked"] = flushes_checked
    d.lii_replay_destroy(rp)
    return log, bytes(status), clouds


@pytest.mark.gpu
def test_replay_host_with_publishing_on(tmp_path):
    import test_gpu_publish as P
    import test_replay_host as T
    import lidar_imu_init_amd as lii
    from lidar_imu_init_amd.api import lii_pc2_fields
    from harness import synth, wire
    d = T._drv()
    (tmp_path / "config").mkdir()
    (tmp_path / "launch").mkdir()
    (tmp_path / "config" / "replay_test.yaml").write_text(T.YAML)
    (tmp_path / "launch" / "replay_test.launch").write_text(T.LAUNCH)
    launch = str(tmp_path / "launch" / "replay_test.launch")
    hall = synth.Hall(size=(24.0, 18.0, 6.0), n_boxes=8, seed=7)
    traj = synth.Trajectory()
    msg_period, n_msgs = 0.1, 230
    R_LI = synth.rot_zyx(np.deg2rad(2.0), np.deg2rad(-1.0), np.deg2rad(-45.0))
    T_LI = np.array([0.05, -0.03, 0.10])
    b_g, b_a, t_off = np.array([-0.001, 0.0015, 0.0005]), np.array([0.004, 0.005, -0.006]), 0.02
    imu = synth.simulate_imu(traj, -0.5, n_msgs * msg_period + 0.5, 200.0, R_LI, T_LI, b_g, b_a, t_off)
    f = wire.pc2_fields(wire.OUSTER)
    msgs = []
    for k in range(n_msgs):
        stamp = k * msg_period
        scan = synth.make_distorted_scan(hall, "mid16k", traj, stamp, msg_period, noise=0.01, seed=3000 + k, blind=0.0)
        raw = wire.pack_pcl2(wire.OUSTER, scan[:, :3], np.zeros(len(scan), np.int32), scan[:, 3].astype(np.float64), stamp)
        msgs.append((stamp, np.frombuffer(raw, np.uint8).copy(), len(scan)))
    log_off, status_off, _ = _run(d, T, launch, msgs, imu, lii_pc2_fields(*f), msg_period, False)
    log_on, status_on, clouds = _run(d, T, launch, msgs, imu, lii_pc2_fields(*f), msg_period, True)
    assert len(log_on) == len(log_off) > 200
    assert log_on.tobytes() == log_off.tobytes()
    assert status_on == status_off
    # the last scan: body cloud = the de-skewed scan, dense cloud = its transform at the logged state
    st = lii.State()
    st.pod[:36] = log_on[-1, 4:40]
    assert len(clouds["scan"]) > 1000
    assert np.array_equal(P._bits(clouds[BODY]), P._bits(clouds["scan"]))
    assert np.array_equal(P._bits(clouds[DENSE]), P._bits(P._to_world(st, clouds["scan"])))
    assert len(clouds[EFFECT]) == int(log_on[-1, 3]) and 0 < len(clouds[EFFECT]) <= len(clouds[DOWN]) <= len(clouds["scan"])
    # the flushes (checked inside the run, spin by spin): every SAVE_INTERVAL registered scans, each ending with the dense cloud of its last scan
    print(f"rows {len(log_on)}, flushes checked against their last scan {clouds['flushes_checked']}, last flush {len(clouds[0])} points")
    assert clouds["flushes_checked"] >= 10 and len(clouds[0]) > 0
