"""IMU forward propagation on the device (lii_imu.hip: k_imu_propagate / k_cv_propagate; lii_imu_propagate, lii_cv_propagate,
lii_scan_register_imu) against the UNMODIFIED reference header - ImuProcess::Process, src/IMU_Processing.hpp:419-461 - as recorded in
tests/golden/imu/reference_propagation.npz (always) and as oracle/_ref/libref_imu.so computes it live (where it is built).

Bounds: the ones tests/test_replay_host.py:100-105 holds the host restatement to against the same header - pose count equal; poses,
state[:36], carry within 1e-12 absolute; max |dcov| <= 1e-12 max |cov|.  Measured maxima: profiles/imu_propagate.md."""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
FIXTURE = os.path.join(ROOT, "tests", "golden", "imu", "reference_propagation.npz")
MEAN_ACC_NORM = 9.805
LIO_CASES = ("n20_end_after", "n11_end_before", "n2_end_after", "skip3", "n63", "far100", "noise_axes")
# the scan-level tests run with noise that differs between gyro and accelerometer and from axis to axis: a swapped or transposed use shows
COV_GYR, COV_ACC = np.array([0.1, 0.2, 0.3]), np.array([0.4, 0.5, 0.6])
CV_CASES = ("dt0.05", "dt0.1", "dt0.013")


def _ref_lib():
    from oracle import oracle as O
    return O if O.ref_imu_lib() is not None else None


def _registrar(**kw):
    import lidar_imu_init_amd as lii
    reg = lii.Registrar(**{**dict(max_scan_points=20_000, max_map_points=600_000, filter_size_map=0.15), **kw})
    return reg


def _check_propagation(tag, state, poses, carry, ref_state, ref_poses, ref_carry):
    """Prints every figure, then asserts test 1's bounds.  carry: acc_s_last, angvel_last, last_lidar_end_time (7,)."""
    d_poses = float(np.abs(poses - ref_poses).max()) if len(poses) == len(ref_poses) else float("nan")
    d_state = float(np.abs(state[:36] - ref_state[:36]).max())
    d_cov = float(np.abs(state[36:] - ref_state[36:]).max() / np.abs(ref_state[36:]).max())
    d_carry = float(np.abs(carry - ref_carry).max())
    print(f"{tag}: K {len(poses)} / {len(ref_poses)}  max|dposes| {d_poses:.2e}  max|dstate[:36]| {d_state:.2e}  max|dcov|/max|cov| {d_cov:.2e}  "
          f"max|dcarry| {d_carry:.2e}")
    assert len(poses) == len(ref_poses)
    assert np.allclose(poses, ref_poses, rtol=0, atol=1e-12)
    assert np.allclose(state[:36], ref_state[:36], rtol=0, atol=1e-12)
    assert np.abs(state[36:] - ref_state[36:]).max() <= 1e-12 * np.abs(ref_state[36:]).max()
    assert np.allclose(carry[:6], ref_carry[:6], rtol=0, atol=1e-12) and abs(carry[6] - ref_carry[6]) < 1e-12
    return d_poses, d_state, d_cov, d_carry


def _carry7(c):
    return np.r_[c["acc_s_last"], c["angvel_last"], c["last_lidar_end_time"]]


@pytest.mark.parametrize("name", LIO_CASES)
def test_imu_propagate_equals_the_reference_header(name):
    import lidar_imu_init_amd as lii
    F = np.load(FIXTURE)
    c = {k: F[f"lio/{name}/in/{k}"] for k in ("state", "imu", "last_imu", "last_end", "acc_s_last", "angvel_last", "beg", "pts", "cov_gyr", "cov_acc")}
    refs = [("fixture", F[f"lio/{name}/out/state"], F[f"lio/{name}/out/poses"], F[f"lio/{name}/out/carry"])]
    O = _ref_lib()
    if O is not None:
        import make_imu_fixture as M
        r = M.run_reference_lio(c)
        refs.append(("live header", r["state"], r["poses"], _carry7(r)))
    reg = _registrar(max_scan_points=1000, max_map_points=1000)
    # (cov_gyr / cov_acc are the two the reference wrapper takes; the others keep the constructor's values, as the wrapper leaves them)
    reg.set_imu_noise(cov_gyr=c["cov_gyr"], cov_acc=c["cov_acc"], mean_acc_norm=MEAN_ACC_NORM)
    reg.imu_carry = dict(last_imu=c["last_imu"], acc_s_last=c["acc_s_last"], angvel_last=c["angvel_last"], last_lidar_end_time=float(c["last_end"]))
    beg = float(c["beg"])
    end = beg + float(c["pts"][-1, 3]) / 1000.0
    st, poses = reg.propagate_imu(c["imu"], beg, end, lii.State(c["state"]))
    carry = reg.imu_carry
    assert np.array_equal(carry["last_imu"], c["imu"][-1])  # last_imu_ = meas.imu.back(), :381
    for tag, rs, rp, rc in refs:
        _check_propagation(f"lii_imu_propagate {name} vs {tag}", st.pod, poses, _carry7(carry), rs, rp, rc)
    reg.close()


@pytest.mark.parametrize("name", CV_CASES)
def test_cv_propagate_equals_the_reference_header(name):
    import lidar_imu_init_amd as lii
    F = np.load(FIXTURE)
    c = {k: F[f"cv/{name}/in/{k}"] for k in ("state", "dt", "pts", "cov_gyr_scale", "cov_acc_scale")}
    refs = [("fixture", F[f"cv/{name}/out/state"])]
    if _ref_lib() is not None:
        import make_imu_fixture as M
        refs.append(("live header", M.run_reference_cv(dict(c, dt=float(c["dt"])))))
    reg = _registrar(max_scan_points=1000, max_map_points=1000)
    got = reg.propagate_cv(float(c["dt"]), c["cov_gyr_scale"], c["cov_acc_scale"], lii.State(c["state"]))
    for tag, want in refs:
        d_state = np.abs(got.pod[:36] - want[:36]).max()
        d_cov = np.abs(got.pod[36:] - want[36:]).max() / np.abs(want[36:]).max()
        print(f"lii_cv_propagate {name} vs {tag}: max|dstate[:36]| {d_state:.2e}  max|dcov|/max|cov| {d_cov:.2e}")
        # (the reference computes dt as a difference of absolute stamps: tests/test_replay_host.py:68)
        assert np.allclose(got.pod[:36], want[:36], rtol=0, atol=1e-12)
        assert np.abs(got.pod[36:] - want[36:]).max() <= 1e-12 * np.abs(want[36:]).max()
    reg.close()


# ---------------------------------------------------------------------------------------------------------------------------
class _LioStream:
    """The LIO phase of tests/test_gpu_end_to_end.py (test_lio_phase_tracks_and_refines_extrinsic): 16 k-point sub-frames of a
    spinning sensor on a moving platform, 200 Hz IMU; scans in ascending time order with distinct stamps (so that the reference's
    std::sort leaves the order alone)."""

    def __init__(self, oracle):
        import lidar_imu_init_amd as lii
        from harness import synth
        self.hall = synth.Hall(size=(24.0, 18.0, 6.0), n_boxes=8, seed=7)
        self.traj = synth.Trajectory()
        self.sweep, self.t0 = 0.05, 2.5
        self.R_LI = synth.rot_zyx(np.deg2rad(-1.0), np.deg2rad(-0.3), np.deg2rad(88.0))
        self.T_LI = np.array([-0.02, 0.02, 0.17])
        self.imu = synth.simulate_imu(self.traj, self.t0 - 0.1, self.t0 + 14 * self.sweep, 200.0, self.R_LI, self.T_LI,
                                      np.array([0.002, 0.0007, -0.0004]), np.array([0.006, -0.007, 0.008]), 0.0)
        self.map_pts = self.hall.surface_points(0.15, noise=0.01, seed=7)
        st = lii.State()
        R0, p0 = self.imu_pose(self.t0)
        st.rot_end[:] = R0
        st.pos_end[:] = p0
        st.vel_end[:] = (self.imu_pose(self.t0 + 1e-4)[1] - self.imu_pose(self.t0 - 1e-4)[1]) / 2e-4
        st.offset_R_L_I[:] = oracle.exp_so3(np.deg2rad([0.03, -0.03, 0.03])) @ self.R_LI
        st.offset_T_L_I[:] = self.T_LI + np.array([0.002, -0.002, 0.002])
        st.gravity[:] = [0.0, 0.0, -9.81]
        st.cov[:] = np.diag(np.r_[np.full(6, 1e-4), np.full(6, 1e-4), np.full(3, 1e-2), np.full(9, 1e-5)])
        self.state0 = st
        self.k_imu = int(np.searchsorted(self.imu[0], self.t0, side="right"))  # samples up to t0 belong to the scan before
        t, g, a = self.imu
        self.carry0 = dict(last_imu=np.r_[t[self.k_imu - 1], g[self.k_imu - 1], a[self.k_imu - 1]], acc_s_last=np.zeros(3), angvel_last=np.zeros(3),
                           last_lidar_end_time=self.t0)

    def imu_pose(self, t):
        R_WL, p_WL = self.traj.R(np.array([t]))[0], self.traj.p(np.array([t]))[0]
        R_WI = R_WL @ self.R_LI.T
        return R_WI, p_WL - R_WI @ self.T_LI

    def scan(self, k):
        """(t_beg, scan sorted by time, IMU rows (n, 7) with stamps <= the scan's end)."""
        from harness import synth
        t_beg = self.t0 + k * self.sweep
        s = synth.make_distorted_scan(self.hall, "mid16k", self.traj, t_beg, self.sweep, noise=0.01, seed=5000 + k)
        _, first = np.unique(s[:, 3], return_index=True)
        s = np.ascontiguousarray(s[first])  # ascending, distinct stamps
        t_end = t_beg + float(s[-1, 3]) / 1000.0
        t, g, a = self.imu
        k1 = int(np.searchsorted(t, t_end, side="right"))
        rows = np.c_[t[self.k_imu:k1], g[self.k_imu:k1], a[self.k_imu:k1]]
        self.k_imu = k1
        return t_beg, s, rows


def _header(O, rows, carry, t_beg, state_pod, scan):
    return O.ref_imu_process_lio(rows, carry["last_imu"], carry["last_lidar_end_time"], carry["acc_s_last"], carry["angvel_last"], COV_GYR,
                                 COV_ACC, 9.81, t_beg, state_pod, scan)


def _ulp_diff(a, b):  # tests/test_gpu_scan_ops.py
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def test_scan_register_imu_equals_the_host_fed_path(oracle):
    """One synthetic LIO scan: lii_scan_register_imu against lii_scan_register fed the reference header's pose table and propagated
    state on the same handle, scan and map, and against the oracle chain (header -> oracle voxel filter -> Tree.iekf_update)."""
    import lidar_imu_init_amd as lii
    O = _ref_lib()
    if O is None:
        pytest.skip("oracle/_ref/libref_imu.so not built (needs the reference tree at build time)")
    S = _LioStream(oracle)
    t_beg, scan, rows = S.scan(0)
    ref = _header(O, rows, S.carry0, t_beg, S.state0.pod, scan)
    leaf = 0.1
    reg = _registrar()
    reg.map_build(S.map_pts)
    reg.set_imu_noise(cov_gyr=COV_GYR, cov_acc=COV_ACC, mean_acc_norm=9.81)
    reg.imu_carry = S.carry0
    # ---- the device-fed call
    reg.scan_upload(scan)
    st_a, prop_a, rep_a = reg.register_imu(rows, t_beg, S.state0.copy(), leaf=leaf, max_iterations=5, imu_en=True, scan_sorted=True)
    cloud_a = reg.scan_download(0)
    carry_a = reg.imu_carry
    # ---- the host-fed call: the header's pose table and propagated state
    reg.scan_upload(scan)
    st_b = lii.State(ref["state"])
    rep_b = reg.scan_register(st_b, lii.State(ref["state"]), imu_poses=ref["poses"], leaf=leaf, max_iterations=5, imu_en=True, scan_sorted=True)
    cloud_b = reg.scan_download(0)
    # (a) the de-skewed cloud: the de-skew's bound against the header (2 ulp, tests/test_gpu_scan_ops.py) plus one - 1e-12 in the poses moves
    # a point by ~1e-10 m, which can flip a final rounding and no more
    assert np.array_equal(cloud_a[:, 3], ref["points"][:, 3])
    ulp_ref = _ulp_diff(cloud_a[:, :3], ref["points"][:, :3])
    share = float((cloud_a[:, :3] != cloud_b[:, :3]).mean())
    print(f"de-skewed cloud: device-fed vs header max {ulp_ref.max()} ulp; host-fed vs header max {_ulp_diff(cloud_b[:, :3], ref['points'][:, :3]).max()} ulp; "
          f"share of coordinates that differ between the two GPU runs {share:.2e} (max {_ulp_diff(cloud_a[:, :3], cloud_b[:, :3]).max()} ulp)")
    assert ulp_ref.max() <= 3 and _ulp_diff(cloud_a[:, :3], cloud_b[:, :3]).max() <= 3
    # (b) the same loop
    print("reports:", {k: rep_a[k] for k in ("iterations", "searches", "effect_num")}, {k: rep_b[k] for k in ("iterations", "searches", "effect_num")})
    assert (rep_a["iterations"], rep_a["searches"], rep_a["effect_num"]) == (rep_b["iterations"], rep_b["searches"], rep_b["effect_num"])
    # (d) state_propagated_out and the carry: test 1's bounds against the header
    _check_propagation("state_propagated_out / carry vs header", prop_a.pod, ref["poses"], _carry7(carry_a), ref["state"], ref["poses"], _carry7(ref))
    assert np.array_equal(carry_a["last_imu"], rows[-1])
    # (c) the final state against the oracle chain, bound of tests/test_gpu_headline_parity.py for scans up to 131 072 points
    tree = oracle.Tree("oracle")
    tree.build(S.map_pts)
    body, _ = oracle.voxel_grid(ref["points"], leaf)
    want = tree.iekf_update(body, ref["state"], ref["state"], max_iterations=5, imu_en=True)
    tree.close()
    w = lii.State(want["state"])
    dp = float(np.linalg.norm(w.pos_end - st_a.pos_end))
    dth = float(np.linalg.norm(oracle.log_so3(w.rot_end.T @ st_a.rot_end)))
    d_pe = float(np.abs(w.pod[:24] - st_a.pod[:24]).max())
    d_rest = float(np.abs(w.pod[24:36] - st_a.pod[24:36]).max())
    print(f"final state vs the oracle chain: |dp| {dp:.2e} m |dtheta| {dth:.2e} rad pose+extrinsic {d_pe:.2e} other states {d_rest:.2e}; "
          f"iterations {rep_a['iterations']} / {want['iters']}")
    # ... and the updated covariance - the one output of the chain that depends on the device-propagated P: that file's dcov_rel bound
    d_cov = float(np.abs(st_a.cov - w.cov).max() / np.abs(w.cov).max())
    print(f"updated covariance vs the oracle chain: max|dcov| / max|cov| {d_cov:.2e}")
    assert rep_a["iterations"] == want["iters"]
    assert dp <= 1e-6 and dth <= 1e-7 and d_pe <= 1e-7 and d_rest <= 1e-5
    assert d_cov <= 5e-4
    reg.close()


def test_ten_scans_carry_stays_with_the_header(oracle):
    """Ten consecutive LIO scans through lii_scan_register_imu, the carry left in the handle.  At every scan the header is run from the
    GPU's previous state and the HEADER's previous carry, so nothing compounds: a carry that is not advanced, or advanced from the
    wrong sample, shows at once."""
    O = _ref_lib()
    if O is None:
        pytest.skip("oracle/_ref/libref_imu.so not built (needs the reference tree at build time)")
    S = _LioStream(oracle)
    reg = _registrar()
    reg.map_build(S.map_pts)
    reg.set_imu_noise(cov_gyr=COV_GYR, cov_acc=COV_ACC, mean_acc_norm=9.81)
    reg.imu_carry = S.carry0
    st = S.state0.copy()
    carry_h = dict(S.carry0)
    worst = np.zeros(4)
    for k in range(10):
        t_beg, scan, rows = S.scan(k)
        ref = _header(O, rows, carry_h, t_beg, st.pod, scan)
        dev = reg.device_scan(scan)
        st, prop, rep = reg.register_imu(rows, t_beg, st, leaf=0.1, max_iterations=5, imu_en=True, scan_dev=dev, scan_sorted=True, map_update=True)
        carry_g = reg.imu_carry
        assert np.array_equal(carry_g["last_imu"], rows[-1])
        worst = np.maximum(worst, _check_propagation(f"scan {k} ({len(rows)} samples)", prop.pod, ref["poses"], _carry7(carry_g), ref["state"], ref["poses"],
                                                     _carry7(ref)))
        assert rep["effect_num"] > 100, rep
        carry_h = dict(last_imu=rows[-1], acc_s_last=ref["acc_s_last"], angvel_last=ref["angvel_last"], last_lidar_end_time=ref["last_lidar_end_time"])
    print("ten scans, worst: poses %.2e state %.2e cov (rel) %.2e carry %.2e" % tuple(worst))
    reg.close()


def test_rules_of_the_entry_points(oracle):
    import ctypes as C
    import lidar_imu_init_amd as lii
    from lidar_imu_init_amd import api
    S = _LioStream(oracle)
    t_beg, scan, rows = S.scan(0)
    reg = _registrar()
    reg.map_build(S.map_pts)
    reg.scan_upload(scan)
    kw = dict(leaf=0.1, max_iterations=5, imu_en=True, scan_sorted=True)

    def code(fn):
        with pytest.raises(lii.LIIError) as e:
            fn()
        return e.value.code

    INVALID, CAPACITY, STATE = -1, -4, -5
    # no noise block, then no carry
    assert code(lambda: reg.register_imu(rows, t_beg, S.state0.copy(), **kw)) == STATE
    assert code(lambda: reg.propagate_imu(rows, t_beg, t_beg + 0.05, S.state0)) == STATE
    reg.set_imu_noise(cov_gyr=COV_GYR, cov_acc=COV_ACC, mean_acc_norm=9.81)
    assert code(lambda: reg.register_imu(rows, t_beg, S.state0.copy(), **kw)) == STATE
    with pytest.raises(lii.LIIError):
        reg.imu_carry
    reg.imu_carry = S.carry0
    # n_imu 0 / 64
    assert code(lambda: reg.register_imu(rows[:0], t_beg, S.state0.copy(), **kw)) == INVALID
    assert code(lambda: reg.propagate_imu(rows[:0], t_beg, t_beg + 0.05, S.state0)) == INVALID
    many = np.repeat(rows[:1], 64, axis=0)
    many[:, 0] += 1e-4 * np.arange(64)
    assert code(lambda: reg.register_imu(many, t_beg, S.state0.copy(), **kw)) == CAPACITY
    assert code(lambda: reg.propagate_imu(many, t_beg, t_beg + 0.05, S.state0)) == CAPACITY
    # a job that brings a pose table, or another de-skew
    assert code(lambda: reg.register_imu(rows, t_beg, S.state0.copy(), imu_poses=np.zeros((3, 22)), **kw)) == INVALID
    job = api.lii_scan_job()
    job.struct_size, job.undistort, job.leaf = C.sizeof(api.lii_scan_job), 2, 0.1
    job.opts = api.lii_iekf_opts(5, 1)
    st = S.state0.copy()
    rep = api.lii_iekf_report()
    assert reg.L.lii_scan_register_imu(reg.h, C.byref(job), rows.ctypes.data, len(rows), t_beg, st.pod.ctypes.data, None, C.byref(rep)) == INVALID
    # none of the refused calls touched the carry
    assert np.array_equal(reg.imu_carry["last_imu"], S.carry0["last_imu"]) and reg.imu_carry["last_lidar_end_time"] == S.t0
    # a communicator attached (a one-rank RCCL communicator puts the loop in its three-launch / all-reduce form): single rank only for now
    reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")
    assert code(lambda: reg.register_imu(rows, t_beg, S.state0.copy(), **kw)) == STATE
    assert code(lambda: reg.propagate_imu(rows, t_beg, t_beg + 0.05, S.state0)) == STATE
    assert code(lambda: reg.propagate_cv(0.05, np.full(3, 50.0), np.full(3, 2.0), S.state0)) == STATE
    assert np.array_equal(reg.imu_carry["last_imu"], S.carry0["last_imu"]) and reg.imu_carry["last_lidar_end_time"] == S.t0
    reg.comm_destroy()
    st_p, poses_p = reg.propagate_imu(rows, t_beg, t_beg + float(scan[-1, 3]) / 1000.0, S.state0)
    assert len(poses_p) == len(rows) + 1 and reg.imu_carry["last_lidar_end_time"] > S.t0
    assert np.array_equal(reg.propagate_cv(0.05, np.full(3, 50.0), np.full(3, 2.0), S.state0).pod[12:36], S.state0.pod[12:36])
    reg.imu_carry = S.carry0
    reg.scan_upload(scan)
    st0r, prop0r, _ = reg.register_imu(rows, t_beg, S.state0.copy(), **kw)
    assert np.array_equal(prop0r.pod, st_p.pod)  # the two entry points propagate alike
    reg.imu_carry = S.carry0
    # a job that announces the next scan registers as any other and leaves nothing armed
    dev = reg.device_scan(scan)
    st1, _, rep1 = reg.register_imu(rows, t_beg, S.state0.copy(), scan_dev=dev, next_scan=dev, **kw)
    t0 = time.perf_counter()
    reg.synchronize()
    dt = time.perf_counter() - t0
    print(f"lii_synchronize behind a job with next_scan_dev set: {dt * 1e3:.2f} ms")
    assert dt < 0.5  # (a launch left waiting would hold the stream for LII_PREARM_TIMEOUT_MS = 2 s)
    reg.imu_carry = S.carry0
    reg.scan_upload(scan)
    st2, _, rep2 = reg.register_imu(rows, t_beg, S.state0.copy(), **kw)
    assert np.array_equal(st1.pod, st2.pod) and rep1["iterations"] == rep2["iterations"]
    # a scan that is not declared sorted takes the time-extent reduction: same propagated state, same cloud up to the voxel sums
    reg.imu_carry = S.carry0
    perm = np.random.default_rng(1).permutation(len(scan))
    reg.scan_upload(scan[perm])
    st3, prop3, rep3 = reg.register_imu(rows, t_beg, S.state0.copy(), **dict(kw, scan_sorted=False))
    reg.imu_carry = S.carry0
    reg.scan_upload(scan)
    _, prop2, _ = reg.register_imu(rows, t_beg, S.state0.copy(), **kw)
    assert np.array_equal(prop3.pod, prop2.pod)
    assert np.linalg.norm(st3.pos_end - st2.pos_end) < 1e-5
    reg.close()


def test_profiling_attributes_the_propagation_launch(oracle):
    """The host-fed comparison run takes its pose table and propagated state from lii_imu_propagate (held to the header above), outside
    the profiled call."""
    S = _LioStream(oracle)
    scans = [S.scan(k) for k in range(4)]
    profiles = []
    for device_fed in (True, False):
        reg = _registrar()
        reg.map_build(S.map_pts)
        reg.set_imu_noise(cov_gyr=COV_GYR, cov_acc=COV_ACC, mean_acc_norm=9.81)
        reg.imu_carry = S.carry0
        st = S.state0.copy()
        reg.set_profiling(1)
        reg.set_profiling(3)
        for t_beg, scan, rows in scans:
            reg.scan_upload(scan)
            if device_fed:
                st, _, _ = reg.register_imu(rows, t_beg, st, leaf=0.1, max_iterations=5, imu_en=True, scan_sorted=True)
            else:
                st, poses = reg.propagate_imu(rows, t_beg, t_beg + float(scan[-1, 3]) / 1000.0, st)
                reg.scan_register(st, st.copy(), imu_poses=poses, leaf=0.1, max_iterations=5, imu_en=True, scan_sorted=True)
        reg.synchronize()
        profiles.append(reg.kernel_profile())
        reg.set_profiling(0)
        reg.close()
    (kp_a, n_a), (kp_b, n_b) = profiles
    print("device-fed:", {k: (round(1e3 * ms / max(n, 1), 2), n) for k, (ms, n) in kp_a.items()})
    print("host-fed:  ", {k: (round(1e3 * ms / max(n, 1), 2), n) for k, (ms, n) in kp_b.items()})
    assert n_a == n_b == len(scans)
    assert kp_a["propagate"][1] == len(scans) and kp_b["propagate"][1] == 0
    for k in ("deskew", "voxel", "knn", "fit_search", "fit", "solve"):  # the new path adds one launch and removes none
        assert kp_a[k][1] == kp_b[k][1], (k, kp_a[k], kp_b[k])
