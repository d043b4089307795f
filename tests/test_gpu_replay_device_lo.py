"""The ROS-free C++ host (harness/li_init_replay.cpp) with lii_replay_set_device_imu(rp, 1), LO phase: every LO scan with a map goes
through lii_scan_register_cv (the constant-velocity propagation rides in the de-skew launch), the scan that seeds the map through
lii_cv_propagate + lii_undistort_cv + lii_downsample + lii_map_build_from_scan - on the stream of tests/test_gpu_replay_device_imu.py,
against the same host with the switch off.

lii_replay_device_calls says which calls were made.  The assertions of that file about the run hold (phases, switch to LIO, row counts,
the initialization result within 1 deg / 0.10 m / 5 ms of the truth); the log has the same rows and the same switch scan as the host
run.  The largest LO-row difference is printed without a bound, for that file's reason: the chain feeds each scan's result into the
next and amplifies single roundings (tests/test_gpu_first_divergence.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _run(d, T, launch, msgs, imu, fields, msg_period, device_imu):
    T._bind(d)
    d.lii_replay_set_device_imu.argtypes = [C.c_void_p, C.c_int32]
    d.lii_replay_device_calls.argtypes = [C.c_void_p, C.c_void_p]
    t_imu, gyro, accel = imu
    cfg = T.ReplayConfig(C.sizeof(T.ReplayConfig), 0, 40_000, 600_000, launch.encode(), None, None, 0, 0)
    rp = C.c_void_p()
    assert d.lii_replay_create(C.byref(cfg), C.byref(rp)) == 0
    assert d.lii_replay_set_device_imu(rp, 1 if device_imu else 0) == 0
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
    ST = T._status_type()
    status = ST()
    status.struct_size = C.sizeof(ST)
    assert d.lii_replay_get_status(rp, C.byref(status)) == 0
    calls = (C.c_int32 * 4)()
    assert d.lii_replay_device_calls(rp, calls) == 0
    assert d.lii_replay_device_calls(None, calls) == -1 and d.lii_replay_device_calls(rp, None) == -1
    d.lii_replay_destroy(rp)
    return log, status, dict(register_imu=calls[0], register_cv=calls[1], cv_propagate=calls[2], map_build_from_scan=calls[3])


@pytest.mark.gpu
def test_replay_host_with_the_lo_phase_on_the_device(tmp_path):
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
    log_h, status_h, calls_h = _run(d, T, launch, msgs, imu, lii_pc2_fields(*f), msg_period, False)
    log, status, calls = _run(d, T, launch, msgs, imu, lii_pc2_fields(*f), msg_period, True)
    print("device calls, switch on:", calls, " switch off:", calls_h)
    assert not any(calls_h.values())
    n_lo, n_lio = int((log[:, 1] == 0).sum()), int((log[:, 1] == 1).sum())
    assert calls["register_cv"] > 150
    assert calls["map_build_from_scan"] == 1 and calls["cv_propagate"] == 1
    assert calls["register_imu"] > 30
    # ---- what the host-IMU test asserts of its run
    assert status.data_accum_start and status.data_accum_finished and status.imu_en and status.refine_done
    assert status.cut_frame_num == 2
    assert n_lo > 150 and n_lio > 30, (n_lo, n_lio)
    R_est = np.array(status.init.R_LI[:]).reshape(3, 3)
    ang = np.rad2deg(np.arccos(np.clip((np.trace(R_LI.T @ R_est) - 1) / 2, -1, 1)))
    assert ang < 1.0 and np.linalg.norm(np.array(status.init.T_LI[:]) - T_LI) < 0.10
    assert abs(status.init_total_time_lag - (t_off - msg_period / 2 / 2)) < 0.005
    # ---- against the run with the switch off: the same rows, the same switch scan
    assert len(log) == len(log_h)
    assert np.array_equal(log[:, 1], log_h[:, 1])
    assert np.allclose(log[:, 0], log_h[:, 0], rtol=0, atol=1e-9)
    dd = np.abs(log[:, 4:] - log_h[:, 4:])
    lo = log[:, 1] == 0
    print(f"device LO vs host LO over {n_lo} LO rows: largest row difference {dd[lo].max():.3e} (rot {dd[lo][:, 0:9].max():.3e}, "
          f"pos {dd[lo][:, 9:12].max():.3e} m); first row that differs at all: {int(np.argmax(dd.max(axis=1) > 0)) if dd.max() > 0 else -1}")
