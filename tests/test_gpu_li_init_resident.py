"""LI-Init resident on the device (lii_li_init_resident, lii_li_init_resident_fetch, lii_calib_solve_stage_dev;
lii_li_init_resident.hip) against the numpy oracle (oracle/li_init_np.py) and against the host chain (lii_li_init_run).

Inputs (tests/li_init_shapes.py, tests/li_init_fixture.py): the reference's committed run (1 369 states), synthetic accumulations of 400
and 900 states, one of 230 states in raw form (every IMU sample, interpolate = 1), short_accumulation(108) - exactly 61 states left for
the second filter - and short_accumulation(112), which every chain refuses.  The oracle's iteration counts on them, run on the CPU:
7 / 3 / 3, 5 / 2 / 24, 4 / 2 / 30, 5 / 3 / 24, 14 / 10 / 15.

Tolerances.  Sequences: the existing chain test's 1e-12 * max(1, max |want|).  Solved parameters on the reference run: those of
test_li_initialization_end_to_end_on_reference_run.  On the other inputs stage 3 takes 15 - 30 steps with b_a on its bounds, so the
bound per quantity is max(that tolerance, 2 * |lii_li_init_run - oracle|): the parent's code against the oracle, the code under test on
neither side, and the factor 2 the solver test grants for "differs in summation order only".  Measured: profiles/li_init_resident.md."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import li_init_fixture as F
import li_init_shapes as S

pytestmark = pytest.mark.gpu

LII_ERR_INVALID, LII_ERR_CAPACITY, LII_ERR_STATE = -1, -4, -5
RES_FIELDS = ("R_LI", "T_LI", "gyro_bias", "acc_bias", "grav_L0", "final_cost", "iterations")
# test_li_initialization_end_to_end_on_reference_run's tolerances
TOL = dict(R_LI=1e-8, gyro_bias=1e-9, time_lag_2=1e-9, total=1e-9, T_LI=1e-7, acc_bias=1e-8, grav_L0=1e-7)


@pytest.fixture(scope="module")
def reg():
    import lidar_imu_init_amd as lii
    r = lii.Registrar(max_scan_points=1000, max_map_points=1000)
    yield r
    r.close()


def _fresh():
    import lidar_imu_init_amd as lii
    return lii.Registrar(max_scan_points=1000, max_map_points=1000)


def _refused(code, call, *args, **kw):
    import lidar_imu_init_amd as lii
    with pytest.raises(lii.LIIError) as e:
        call(*args, **kw)
    assert e.value.code == code, (e.value.code, code)
    return True


# ------------------------------------------------------------------------------------------------ inputs and their oracle results
def _raw_accumulation(n_states=230, seed=51, rate=20.0):
    """synthetic_accumulation's recipe (tests/li_init_shapes.py) without its call of lii_li_init_interpolate: every LiDAR-odometry
    state and every sample of the simulated 200 Hz IMU.  Returns (imu_all22, lidar22, move_start_time)."""
    from harness import synth
    from lidar_imu_init_amd import calib_state_array
    rng = np.random.default_rng(seed)
    traj = synth.Trajectory()
    dt = 1.0 / rate
    ts = dt * np.arange(1, n_states + 1)
    lid = calib_state_array(n_states)
    lid[:, 0:9] = traj.R(ts).reshape(-1, 9)
    lid[:, 9:12] = traj.omega_body(ts - dt / 2) + rng.normal(0, 0.01, (n_states, 3))
    lid[:, 12:15] = traj.vel(ts) + rng.normal(0, 0.01, (n_states, 3))
    lid[:, 21] = ts
    R_LI = synth.rot_zyx(np.deg2rad(-1.0), np.deg2rad(-0.3), np.deg2rad(88.0))
    t_imu, gyro, accel = synth.simulate_imu(traj, -0.5, ts[-1] + 0.5, 200.0, R_LI, np.array([-0.02, 0.02, 0.17]),
                                            np.array([0.002, 0.0007, -0.0004]), np.array([0.006, -0.007, 0.008]), 0.015, seed=seed)
    imu_all = calib_state_array(len(t_imu))
    imu_all[:, 9:12], imu_all[:, 18:21], imu_all[:, 21] = gyro, accel, t_imu
    return imu_all, lid, 2.5


_inputs, _oracle = {}, {}


def _input(name):
    """name -> dict(imu, lid (n x 22), freq, cut, interpolate, mst)"""
    if name not in _inputs:
        if name == "reference":
            imu, lid = F.sequences()
            _inputs[name] = dict(imu=imu.to_records(), lid=lid.to_records(), freq=10, cut=5, interpolate=False, mst=0.0)
        elif name in ("acc400", "acc900"):
            imu22, lid22 = S.synthetic_accumulation(int(name[3:]))
            _inputs[name] = dict(imu=imu22, lid=lid22, freq=20, cut=1, interpolate=False, mst=0.0)
        elif name == "raw230":
            imu_all, lid, mst = _raw_accumulation()
            _inputs[name] = dict(imu=imu_all, lid=lid, freq=20, cut=1, interpolate=True, mst=mst)
        else:
            imu, lid = S.short_accumulation(int(name[5:]))
            _inputs[name] = dict(imu=imu.to_records(), lid=lid.to_records(), freq=10, cut=5, interpolate=False, mst=0.0)
    return _inputs[name]


def _want(name):
    """The oracle's LI_Initialization on the input, computed once per process and left unchanged."""
    if name not in _oracle:
        from oracle import li_init_np as LI
        if name == "reference":
            out = dict(F.run(solve=True))
            out["n_aligned"] = len(_input(name)["imu"])
        else:
            x = _input(name)
            imu, lid = S.seq_from_records(x["imu"]), S.seq_from_records(x["lid"])
            if x["interpolate"]:
                imu, lid = LI.downsample_interpolate_imu(imu, lid, x["mst"])
            out = LI.li_initialization(imu, lid, x["freq"], x["cut"])
            out["n_aligned"] = len(imu)
        _oracle[name] = out
    return _oracle[name]


def _resident(reg, name):
    x = _input(name)
    return reg.li_init_resident(x["imu"], x["lid"], x["freq"], x["cut"], interpolate=x["interpolate"], move_start_time=x["mst"])


def _res_bytes(res):
    return b"".join(np.array(getattr(res, f)[:]).tobytes() for f in RES_FIELDS) + np.array([res.time_lag_2]).tobytes()


def _rep_bytes(rep):
    return bytes(rep)


def _quantities(res, total):
    return dict(R_LI=np.array(res.R_LI[:]), gyro_bias=np.array(res.gyro_bias[:]), time_lag_2=np.array([res.time_lag_2]),
                total=np.array([total]), T_LI=np.array(res.T_LI[:]), acc_bias=np.array(res.acc_bias[:]), grav_L0=np.array(res.grav_L0[:]))


def _oracle_quantities(out):
    return dict(R_LI=out["stage2"]["R_LI"].reshape(-1), gyro_bias=out["stage2"]["gyro_bias"], time_lag_2=np.array([out["stage2"]["time_lag_2"]]),
                total=np.array([out["time_delay"]]), T_LI=out["stage3"]["T_LI"], acc_bias=out["stage3"]["acc_bias"], grav_L0=out["stage3"]["grav_L0"])


# ------------------------------------------------------------------------------------------------ 1. the device LM alone
@pytest.mark.parametrize("n", (257, 700))
def test_device_lm_follows_the_oracle(reg, n):
    """n = 257: two records on lane 0 of the evaluator, one on every other; n = 700: the host LM's existing case."""
    from lidar_imu_init_amd.api import lii_calib_result
    from oracle import li_init_np as LI
    if n == 700:
        o = S.oracle_solution()
        imu, lid, truth, s1, s2, s3, oerr = o["imu"], o["lid"], o["truth"], o["s1"], o["s2"], o["s3"], o["err"]
    else:
        imu, lid, truth = S.solver_problem(n=n)
        s1 = LI.solve_stage1(imu, lid)
        s2 = LI.solve_stage2(imu, lid, s1["R_LI"])
        s3 = LI.solve_stage3(imu, lid, s2["R_LI"])
        oerr = S.recovery_errors(truth, s2["R_LI"], s2["gyro_bias"], s2["time_lag_2"], s3["T_LI"], s3["acc_bias"], s3["grav_L0"])
    reg.calib_set_buffers(imu.to_records(), lid.to_records())
    res = lii_calib_result()
    res.R_LI[:] = list(np.eye(3).reshape(-1))
    reg.calib_solve_stage_dev(1, res)
    assert np.allclose(np.array(res.R_LI[:]).reshape(3, 3), s1["R_LI"], atol=1e-8)
    assert res.iterations[0] == s1["iterations"]
    reg.calib_solve_stage_dev(2, res)
    assert np.allclose(np.array(res.R_LI[:]).reshape(3, 3), s2["R_LI"], atol=1e-8)
    assert np.allclose(res.gyro_bias[:], s2["gyro_bias"], atol=1e-9)
    assert abs(res.time_lag_2 - s2["time_lag_2"]) < 1e-9
    assert res.iterations[1] == s2["iterations"]
    reg.calib_solve_stage_dev(3, res)
    print(f"n {n}: iterations {res.iterations[:]} oracle {[s1['iterations'], s2['iterations'], s3['iterations']]}; "
          f"|T_LI - oracle| {np.abs(np.array(res.T_LI[:]) - s3['T_LI']).max():.2e} acc_bias {np.abs(np.array(res.acc_bias[:]) - s3['acc_bias']).max():.2e} "
          f"grav_L0 {np.abs(np.array(res.grav_L0[:]) - s3['grav_L0']).max():.2e}")
    assert np.allclose(res.T_LI[:], s3["T_LI"], atol=1e-8)
    assert np.allclose(res.acc_bias[:], s3["acc_bias"], atol=1e-9)
    assert np.allclose(res.grav_L0[:], s3["grav_L0"], atol=1e-8)
    assert res.iterations[2] == s3["iterations"]
    err = S.recovery_errors(truth, res.R_LI[:], res.gyro_bias[:], res.time_lag_2, res.T_LI[:], res.acc_bias[:], res.grav_L0[:])
    print("recovery error, device LM:", err, "oracle:", oerr)
    for key, e in err.items():
        assert e <= 2.0 * oerr[key], key


# ------------------------------------------------------------------------------------------------ 2. the chain's bits
@pytest.mark.parametrize("name", ("reference", "acc400", "acc900", "raw230", "short108"))
def test_chain_leaves_the_oracles_sequences(reg, name):
    want = _want(name)
    res, rep = _resident(reg, name)
    assert rep.n_aligned == want["n_aligned"]
    assert rep.lag_samples == want["lag_frames"] and rep.time_lag_1 == want["time_lag_1"]
    for which, ki, kl, n_rep in ((1, "imu_stage12", "lidar_stage12", rep.n_stage12), (2, "imu_stage3", "lidar_stage3", rep.n_stage3)):
        gi, gl = reg.li_init_resident_fetch(which)
        wi, wl = want[ki].to_records(), want[kl].to_records()
        assert len(gi) == len(wi) == n_rep and len(gl) == len(wl)
        for g, w, who in ((gi, wi, "imu"), (gl, wl, "lidar")):
            d = np.max(np.abs(g - w))
            tol = 1e-12 * max(1.0, np.max(np.abs(w)))
            print(f"{name} fetch({which}) {who}: {len(g)} states, max |got - want| {d:.3e} (bound {tol:.3e}), equal bits: {np.array_equal(g, w)}")
            assert d <= tol, (name, which, who)


@pytest.mark.parametrize("name", ("reference", "acc400", "acc900"))
def test_both_chains_leave_the_same_stage3_buffers(reg, name):
    """Aligned form, one handle: lii_li_init_run (host chain) then lii_calib_eval(3, p), lii_li_init_resident then lii_calib_eval(3, p)."""
    x = _input(name)
    rng = np.random.default_rng(7)
    p = S.pack_params(3, S.rand_rot(rng), np.r_[rng.normal(0, 0.005, 3), rng.normal(0, 0.2, 3)], S.rand_rot(rng))
    reg.li_init_set_device(False)
    res_h, lag_h, tot_h = reg.li_init_run(x["imu"], x["lid"], x["freq"], x["cut"])
    eh = S.flat(*reg.calib_eval(3, p))
    res_r, rep = _resident(reg, name)
    er = S.flat(*reg.calib_eval(3, p))
    assert rep.time_lag_1 == lag_h
    print(f"{name}: time_lag_2 host {res_h.time_lag_2!r} resident {res_r.time_lag_2!r}; max |eval difference| {np.max(np.abs(eh - er)):.3e}")
    assert eh.tobytes() == er.tobytes()


# ------------------------------------------------------------------------------------------------ 3. one evaluator
def test_the_lm_and_calib_eval_share_one_evaluator(reg):
    res, rep = _resident(reg, "acc400")
    _, _, cost = reg.calib_eval(3, np.array(rep.params[2][:]))
    assert np.float64(cost).tobytes() == np.float64(res.final_cost[2]).tobytes()
    imu12, lid12 = reg.li_init_resident_fetch(1)
    reg.calib_set_buffers(imu12, lid12)
    for stage, np_ in ((1, 9), (2, 13)):
        _, _, cost = reg.calib_eval(stage, np.array(rep.params[stage - 1][:np_]))
        assert np.float64(cost).tobytes() == np.float64(res.final_cost[stage - 1]).tobytes(), stage


# ------------------------------------------------------------------------------------------------ 4. the whole call
def test_whole_call_on_the_reference_run(reg):
    from oracle import oracle as O
    d = F.load()
    out = _want("reference")
    res, rep = _resident(reg, "reference")
    assert res.iterations[:] == [7, 3, 3] == [out["stage1"]["iterations"], out["stage2"]["iterations"], out["stage3"]["iterations"]]
    assert (rep.n_stage12, rep.n_stage3, rep.lag_samples) == (1333, 1332, -4)
    assert abs(rep.time_lag_1 - out["time_lag_1"]) < 1e-15 and abs(rep.time_lag_1 + 0.08) < 1e-12
    got, want = _quantities(res, rep.total_time_lag), _oracle_quantities(out)
    for k in TOL:
        dk = np.max(np.abs(got[k] - want[k]))
        print(f"reference run {k}: |resident - oracle| {dk:.3e} (tolerance {TOL[k]:.0e})")
        assert dk <= TOL[k], k
    R = np.array(res.R_LI[:]).reshape(3, 3)
    assert np.abs(O.rot_to_euler(R) * 57.3 - d["result_rot_euler_deg"]).max() < 0.01
    assert np.abs(np.array(res.T_LI[:]) - d["result_trans"]).max() < 1e-3
    assert np.abs(np.array(res.acc_bias[:]) - d["result_acc_bias"]).max() < 1e-5
    print(f"terminations {rep.termination[:]}, launches {rep.launches}, host waits {rep.host_waits}")


@pytest.mark.parametrize("name", ("acc400", "acc900", "short108"))
def test_whole_call_against_the_oracle_and_the_host_chain(reg, name):
    x = _input(name)
    want = _oracle_quantities(_want(name))
    reg.li_init_set_device(False)
    res_h, lag_h, tot_h = reg.li_init_run(x["imu"], x["lid"], x["freq"], x["cut"])
    res_r, rep = _resident(reg, name)
    host, got = _quantities(res_h, tot_h), _quantities(res_r, rep.total_time_lag)
    o = _want(name)
    print(f"{name}: iterations resident {res_r.iterations[:]} host {res_h.iterations[:]} "
          f"oracle {[o['stage1']['iterations'], o['stage2']['iterations'], o['stage3']['iterations']]}; terminations {rep.termination[:]}")
    worst = []
    for k in TOL:
        d_host = np.max(np.abs(host[k] - want[k]))
        d_res = np.max(np.abs(got[k] - want[k]))
        bound = max(TOL[k], 2.0 * d_host)
        print(f"{name} {k}: |host - oracle| {d_host:.3e}  |resident - oracle| {d_res:.3e}  |resident - host| {np.max(np.abs(got[k] - host[k])):.3e}  bound {bound:.3e}")
        if d_res > bound:
            worst.append(k)
    assert not worst, worst
    assert res_r.iterations[:] == res_h.iterations[:]


# ------------------------------------------------------------------------------------------------ 5. rules
def test_argument_errors_on_a_live_handle(reg):
    x = _input("acc400")
    imu, lid = x["imu"], x["lid"]
    assert _refused(LII_ERR_INVALID, reg.li_init_resident, imu[:199], lid[:199], 20, 1)
    assert _refused(LII_ERR_INVALID, reg.li_init_resident, imu, lid[:-1], 20, 1)
    assert _refused(LII_ERR_INVALID, reg.li_init_resident, imu[:5], lid, 20, 1, interpolate=True)
    assert _refused(LII_ERR_INVALID, reg.li_init_resident, imu, lid[:0], 20, 1, interpolate=True)
    assert _refused(LII_ERR_INVALID, reg.li_init_resident, imu, lid, 0, 1)
    assert _refused(LII_ERR_INVALID, reg.li_init_resident, imu, lid, 20, 0)
    from lidar_imu_init_amd import api
    out = api.lii_calib_result()
    job = api.lii_li_init_job(C.sizeof(api.lii_li_init_job), 2, imu.ctypes.data, len(imu), lid.ctypes.data, len(lid), 0.0, 20, 1)
    assert reg.L.lii_li_init_resident(reg.h, C.byref(job), C.byref(out), None) == LII_ERR_INVALID
    job.interpolate, job.struct_size = 0, 8
    assert reg.L.lii_li_init_resident(reg.h, C.byref(job), C.byref(out), None) == LII_ERR_INVALID
    assert reg.L.lii_li_init_resident(reg.h, None, C.byref(out), None) == LII_ERR_INVALID
    # raw form whose interpolation leaves fewer than 200 states: found on the device
    raw, rlid, mst = _raw_accumulation()
    assert _refused(LII_ERR_INVALID, reg.li_init_resident, raw, rlid[:150], 20, 1, interpolate=True, move_start_time=mst)
    res, rep = _resident(reg, "acc400")  # the handle stays usable; rep == NULL is accepted
    job = api.lii_li_init_job(C.sizeof(api.lii_li_init_job), 0, imu.ctypes.data, len(imu), lid.ctypes.data, len(lid), 0.0, 20, 1)
    assert reg.L.lii_li_init_resident(reg.h, C.byref(job), C.byref(out), None) == 0
    assert _res_bytes(out) == _res_bytes(res)


def test_refusal_found_on_the_device_leaves_the_handle_usable():
    import lidar_imu_init_amd as lii
    r = _fresh()
    try:
        assert _refused(LII_ERR_STATE, r.li_init_resident_fetch, 1)  # no resident run yet
        imu, lid = S.short_accumulation(112)  # 58 states left for the second filter
        with pytest.raises(lii.LIIError) as e:
            r.li_init_resident(imu.to_records(), lid.to_records(), 10, 5)
        assert e.value.code == LII_ERR_INVALID and "fewer than 61 aligned states left to filter" in str(e.value)
        assert _refused(LII_ERR_STATE, r.li_init_resident_fetch, 1)  # a refused run serves no sequences
        res, rep = _resident(r, "short108")
        assert (rep.n_stage12, rep.n_stage3) == (61, 61) and rep.time_lag_1 == -108 / 50.0
        want = _oracle_quantities(_want("short108"))
        assert np.allclose(res.R_LI[:], want["R_LI"], atol=1e-6)  # (held to its bound in test_whole_call_against_the_oracle_and_the_host_chain)
        n = C.c_int32(0)
        buf = np.zeros((60, 22))
        rc = r.L.lii_li_init_resident_fetch(r.h, 1, buf.ctypes.data, buf.ctypes.data, 60, C.byref(n))
        assert rc == LII_ERR_CAPACITY and n.value == 61 and not buf.any()
        assert r.L.lii_li_init_resident_fetch(r.h, 3, None, None, 0, C.byref(n)) == LII_ERR_INVALID
    finally:
        r.close()


def test_launches_and_waits_do_not_depend_on_the_input(reg):
    reps = [_resident(reg, name)[1] for name in ("reference", "acc400", "short108")]
    assert all(rep.host_waits == 1 for rep in reps)
    assert len({rep.launches for rep in reps}) == 1 and reps[0].launches > 0
    print("launches per call:", reps[0].launches)


def test_repeated_and_shrinking_inputs_return_a_fresh_handles_bytes():
    def everything(r, name):
        res, rep = _resident(r, name)
        return (_res_bytes(res), _rep_bytes(rep)) + tuple(a.tobytes() for w in (1, 2) for a in r.li_init_resident_fetch(w))

    fresh = {}
    for name in ("acc900", "acc400"):
        r = _fresh()
        try:
            fresh[name] = everything(r, name)
            assert everything(r, name) == fresh[name], "two identical calls return identical bytes"
        finally:
            r.close()
    r = _fresh()
    try:
        for name in ("acc900", "acc400", "acc900"):  # no stale tail of the longer run is read
            assert everything(r, name) == fresh[name], name
        # lii_li_init_run on that handle still returns its own bits, with either chain
        x = _input("acc400")
        q = _fresh()
        try:
            q.li_init_set_device(False)
            res_q, lag_q, tot_q = q.li_init_run(x["imu"], x["lid"], x["freq"], x["cut"])
        finally:
            q.close()
        for on in (False, True):
            r.li_init_set_device(on)
            res, lag, tot = r.li_init_run(x["imu"], x["lid"], x["freq"], x["cut"])
            assert _res_bytes(res) == _res_bytes(res_q) and (lag, tot) == (lag_q, tot_q), on
        r.li_init_set_device(False)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 6. the replay host
def _replay(d, T, launch, msgs, imu, fields, msg_period, resident):
    T._bind(d)
    d.lii_replay_set_li_init_resident.argtypes = [C.c_void_p, C.c_int32]
    d.lii_replay_li_init_report.argtypes = [C.c_void_p, C.c_void_p]
    t_imu, gyro, accel = imu
    cfg = T.ReplayConfig(C.sizeof(T.ReplayConfig), 0, 40_000, 600_000, launch.encode(), None, None, 1, 0)  # stop_after_init
    rp = C.c_void_p()
    assert d.lii_replay_create(C.byref(cfg), C.byref(rp)) == 0
    assert d.lii_replay_set_li_init_resident(rp, 1 if resident else 0) == 0
    ST = T._status_type()
    status = ST()
    status.struct_size = C.sizeof(ST)
    k_imu = 0
    for stamp, raw, n in msgs:
        while k_imu < len(t_imu) and t_imu[k_imu] <= stamp + msg_period:
            g, a = np.ascontiguousarray(gyro[k_imu]), np.ascontiguousarray(accel[k_imu])
            assert d.lii_replay_imu(rp, float(t_imu[k_imu]), T._dp(g), T._dp(a)) == 0
            k_imu += 1
        assert d.lii_replay_pcl2(rp, stamp, raw.ctypes.data_as(C.c_void_p), n, C.byref(fields)) == 0
        rc = d.lii_replay_spin(rp)
        assert rc >= 0, d.lii_replay_last_error(rp)
        assert d.lii_replay_get_status(rp, C.byref(status)) == 0
        if status.data_accum_finished:
            break
    from lidar_imu_init_amd import api
    rep = api.lii_li_init_report()
    rc = d.lii_replay_li_init_report(rp, C.byref(rep))
    assert rc == (0 if resident else LII_ERR_STATE)
    d.lii_replay_destroy(rp)
    return status, rep


def test_replay_host_with_the_resident_initialization(tmp_path):
    """The stream of tests/test_replay_host.py::test_replay_host_runs_lo_li_init_lio_like_the_python_harness (Ouster layout, the
    shortest replay input of the suite that reaches LI-Init), fed until the initialization result exists, with the switch off and on:
    the same lag of the cross-correlation, and a calibration within the reference-run tolerances of the off-run's - which is inside
    what rule 4 of the module docstring allows, whatever the host chain's distance to the oracle is."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
    imu = synth.simulate_imu(traj, -0.5, n_msgs * msg_period + 0.5, 200.0, R_LI, np.array([0.05, -0.03, 0.10]),
                             np.array([-0.001, 0.0015, 0.0005]), np.array([0.004, 0.005, -0.006]), 0.02)
    f = wire.pc2_fields(wire.OUSTER)
    msgs = []
    for k in range(n_msgs):
        stamp = k * msg_period
        scan = synth.make_distorted_scan(hall, "mid16k", traj, stamp, msg_period, noise=0.01, seed=3000 + k, blind=0.0)
        raw = wire.pack_pcl2(wire.OUSTER, scan[:, :3], np.zeros(len(scan), np.int32), scan[:, 3].astype(np.float64), stamp)
        msgs.append((stamp, np.frombuffer(raw, np.uint8).copy(), len(scan)))
    off, _ = _replay(d, T, launch, msgs, imu, lii_pc2_fields(*f), msg_period, False)
    on, rep = _replay(d, T, launch, msgs, imu, lii_pc2_fields(*f), msg_period, True)
    assert off.data_accum_finished and on.data_accum_finished and on.scans_processed == off.scans_processed
    assert on.init_time_lag_1 == off.init_time_lag_1 == rep.time_lag_1
    assert rep.lag_samples == round(off.init_time_lag_1 * 10 * 2)  # orig_odom_freq 10, cut_frame_num 2
    assert rep.host_waits == 1
    a, b = _quantities(on.init, on.init_total_time_lag), _quantities(off.init, off.init_total_time_lag)
    print(f"replay: {rep.n_aligned} aligned states, lag {rep.lag_samples} samples, iterations resident {on.init.iterations[:]} host {off.init.iterations[:]}")
    for k in TOL:
        dk = np.max(np.abs(a[k] - b[k]))
        print(f"replay {k}: |resident - host chain| {dk:.3e} (tolerance {TOL[k]:.0e})")
        assert dk <= TOL[k], k
    assert on.init.iterations[:] == off.init.iterations[:]
