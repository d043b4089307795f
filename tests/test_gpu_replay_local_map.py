"""The ROS-free C++ host (harness/li_init_replay.cpp) with lii_replay_set_local_map(rp, 1): cube_side_length / mapping/det_range of the
launch file go to lii_local_map_set before the first scan; with lii_replay_set_device_imu the registration calls segment by themselves,
the scan that seeds the map and every scan of the host-propagated path call lii_local_map_segment.  The test stream's cube (2 000 m)
never moves, so the log must keep the bits it has with the switch off - on both paths - while lii_local_map_get shows the cube placed
around the first propagated position and one call per processed scan doing nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _run(d, T, launch, msgs, imu, fields, msg_period, device_imu, local_map):
    from lidar_imu_init_amd import api
    T._bind(d)
    d.lii_replay_set_device_imu.argtypes = [C.c_void_p, C.c_int32]
    d.lii_replay_set_local_map.argtypes = [C.c_void_p, C.c_int32]
    d.lii_replay_handle.restype = C.c_void_p
    d.lii_replay_handle.argtypes = [C.c_void_p]
    t_imu, gyro, accel = imu
    cfg = T.ReplayConfig(C.sizeof(T.ReplayConfig), 0, 40_000, 600_000, launch.encode(), None, None, 0, 0)
    rp = C.c_void_p()
    assert d.lii_replay_create(C.byref(cfg), C.byref(rp)) == 0
    assert d.lii_replay_set_device_imu(rp, 1 if device_imu else 0) == 0
    assert d.lii_replay_set_local_map(None, 1) == -1
    assert d.lii_replay_set_local_map(rp, 1 if local_map else 0) == 0
    k_imu = 0
    for stamp, raw, n in msgs:
        while k_imu < len(t_imu) and t_imu[k_imu] <= stamp + msg_period:
            g, a = np.ascontiguousarray(gyro[k_imu]), np.ascontiguousarray(accel[k_imu])
            assert d.lii_replay_imu(rp, float(t_imu[k_imu]), T._dp(g), T._dp(a)) == 0
            k_imu += 1
        assert d.lii_replay_pcl2(rp, stamp, raw.ctypes.data_as(C.c_void_p), n, C.byref(fields)) == 0
        rc = d.lii_replay_spin(rp)
        assert rc >= 0, d.lii_replay_last_error(rp)
    n_rows = C.c_int32(0)
    assert d.lii_replay_log(rp, None, 0, C.byref(n_rows)) == 0
    log = np.zeros((n_rows.value, 40))
    assert d.lii_replay_log(rp, log.ctypes.data_as(C.c_void_p), n_rows.value, C.byref(n_rows)) == 0
    info = api.lii_local_map_info()
    L = api.load_library()
    rc = L.lii_local_map_get(C.c_void_p(d.lii_replay_handle(rp)), C.byref(info))
    d.lii_replay_destroy(rp)
    return log, rc, info


@pytest.mark.gpu
@pytest.mark.parametrize("device_imu", [False, True])
def test_replay_host_with_the_local_map(tmp_path, device_imu):
    import test_replay_host as T
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
    msg_period, n_msgs = 0.1, 30
    imu = synth.simulate_imu(traj, -0.5, n_msgs * msg_period + 0.5, 200.0, np.eye(3), np.zeros(3), np.zeros(3), np.zeros(3), 0.0)
    f = wire.pc2_fields(wire.OUSTER)
    msgs = []
    for k in range(n_msgs):
        stamp = k * msg_period
        scan = synth.make_distorted_scan(hall, "mid16k", traj, stamp, msg_period, noise=0.01, seed=3000 + k, blind=0.0)
        raw = wire.pack_pcl2(wire.OUSTER, scan[:, :3], np.zeros(len(scan), np.int32), scan[:, 3].astype(np.float64), stamp)
        msgs.append((stamp, np.frombuffer(raw, np.uint8).copy(), len(scan)))
    log_off, rc_off, _ = _run(d, T, launch, msgs, imu, lii_pc2_fields(*f), msg_period, device_imu, False)
    log_on, rc_on, info = _run(d, T, launch, msgs, imu, lii_pc2_fields(*f), msg_period, device_imu, True)
    assert rc_off == -5  # LII_ERR_STATE: nobody called lii_local_map_set
    assert rc_on == 0 and info.initialized == 1 and info.moves == 0 and info.deleted_total == 0 and info.last_n_boxes == 0
    cube = np.array(info.cube[:])
    print("rows", len(log_on), "cube", cube)
    assert np.allclose(cube[3:] - cube[:3], 2000.0) and np.abs(cube[:3] + 1000.0).max() < 1.0  # placed around the first (propagated) position
    assert len(log_on) == len(log_off) > 30
    assert np.array_equal(log_on.view(np.uint64), log_off.view(np.uint64))
