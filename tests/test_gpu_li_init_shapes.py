"""The LI-Init device code (k_calib_eval<1,2,3>, k_zero_phase, k_xcorr_prepare, k_xcorr, k_xcorr_argmax behind lii_calib_eval,
lii_calib_solve_stage, lii_zero_phase_filter, lii_xcorr_lag, lii_li_init_run) at sizes and inputs beyond the reference's one run:
around the evaluator's 256-lane tree, across k_zero_phase's workgroups, on the argmax kernel's stride boundaries and plateaus.
Inputs, the mpmath reference and the derived bound: tests/li_init_shapes.py; their CPU checks: test_oracle_li_init_shapes.py.
Measured figures: profiles/li_init_shapes.md."""
import numpy as np
import pytest

import li_init_shapes as S

pytestmark = pytest.mark.gpu

LII_ERR_INVALID, LII_ERR_STATE = -1, -5


@pytest.fixture(scope="module")
def reg():
    import lidar_imu_init_amd as lii
    r = lii.Registrar(max_scan_points=1000, max_map_points=1000)
    yield r
    r.close()


def _fresh():
    import lidar_imu_init_amd as lii
    return lii.Registrar(max_scan_points=1000, max_map_points=1000)


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _refused(code, call, *args):
    import lidar_imu_init_amd as lii
    with pytest.raises(lii.LIIError) as e:
        call(*args)
    assert e.value.code == code
    return True


def _eval_all(reg, imu, lid):
    """Every stage at every parameter point on the uploaded buffers: a list of flat output vectors."""
    reg.calib_set_buffers(imu.to_records(), lid.to_records())
    return [S.flat(*reg.calib_eval(stage, S.pack_params(stage, *pt))) for stage in (1, 2, 3) for pt in S.param_points(stage)]


# ------------------------------------------------------------------------------------------------ 1. evaluator
@pytest.mark.parametrize("n", S.EVAL_SIZES)
def test_eval_matches_numpy_oracle(reg, n):
    from oracle import li_init_np as LI
    imu, lid = S.random_pair(n, seed=11)
    reg.calib_set_buffers(imu.to_records(), lid.to_records())
    for stage in (1, 2, 3):
        for R, v, R_LI in S.param_points(stage):
            JtJ, Jtr, cost = reg.calib_eval(stage, S.pack_params(stage, R, v, R_LI))
            rJ, rg, rc = LI.normal_equations(stage, R, v, imu, lid, R_LI)
            print(f"n {n} stage {stage}: JtJ {_rel(JtJ, rJ):.2e} Jtr {_rel(Jtr, rg):.2e} cost {abs(cost - rc) / rc:.2e}")
            assert _rel(JtJ, rJ) < 1e-10 and _rel(Jtr, rg) < 1e-10 and abs(cost - rc) / rc < 1e-12


@pytest.mark.parametrize("stage", (1, 2, 3))
@pytest.mark.parametrize("n", S.MP_SIZES)
def test_eval_within_the_derived_bound_of_the_exact_result(reg, n, stage):
    """|got - exact| <= (ceil(n / 256) + 8 + c) 2^-53 sum_i mag_i per output entry, exact and mag_i from the 60-digit reference
    (tests/li_init_shapes.py: how c = 11 / 15 / 31 is counted and what mag_i is).  Measured worst ratio to the bound on an
    MI355X: see profiles/li_init_shapes.md."""
    imu, lid = S.random_pair(n, seed=11)
    reg.calib_set_buffers(imu.to_records(), lid.to_records())
    for k in range(3):
        imu_r, lid_r, pt, exact, mag = S.reference(stage, n, k)
        assert np.array_equal(imu_r.to_records(), imu.to_records()) and np.array_equal(lid_r.to_records(), lid.to_records())
        got = S.flat(*reg.calib_eval(stage, S.pack_params(stage, *pt)))
        ratio = S.worst_ratio(stage, n, got, exact, mag)
        print(f"n {n} stage {stage} point {k}: worst |got - exact| / bound = {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("n", (257, 4099))
def test_eval_is_deterministic(reg, n):
    imu, lid = S.random_pair(n, seed=12)
    first = _eval_all(reg, imu, lid)
    for a, b in zip(first, _eval_all(reg, imu, lid)):
        assert a.tobytes() == b.tobytes()
    for stage in (1, 2, 3):  # and back to back on the same upload
        p = S.pack_params(stage, *S.param_points(stage)[0])
        assert S.flat(*reg.calib_eval(stage, p)).tobytes() == S.flat(*reg.calib_eval(stage, p)).tobytes()


def test_eval_after_shrink_and_grow_equals_a_fresh_handle():
    """set_buffers keeps the larger allocation when n shrinks: the stale tail (samples 65 .. 4098 of the first set) must not be
    read, and growing again must not keep anything of the small set."""
    sets = [S.random_pair(n, seed) for n, seed in ((4099, 13), (65, 14), (4099, 15))]
    one = _fresh()
    try:
        got = [_eval_all(one, imu, lid) for imu, lid in sets]
    finally:
        one.close()
    for (imu, lid), g in zip(sets, got):
        f = _fresh()
        try:
            want = _eval_all(f, imu, lid)
        finally:
            f.close()
        for a, b in zip(g, want):
            assert a.tobytes() == b.tobytes(), len(imu)


def test_eval_rules():
    r = _fresh()
    try:
        p1 = S.pack_params(1, *S.param_points(1)[0])
        assert _refused(LII_ERR_STATE, r.calib_eval, 1, p1)  # nothing uploaded yet
        imu, lid = S.random_pair(65, seed=16)
        want = _eval_all(r, imu, lid)
        L, h = r.L, r.h
        import ctypes as C
        out = np.zeros(128)
        for stage in (0, 4):
            assert L.lii_calib_eval(h, stage, p1.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), None, None) == LII_ERR_INVALID
        assert _refused(LII_ERR_INVALID, r.calib_set_buffers, np.zeros((0, 22)), np.zeros((0, 22)))
        # the refused calls leave the previous buffers usable
        again = [S.flat(*r.calib_eval(stage, S.pack_params(stage, *pt))) for stage in (1, 2, 3) for pt in S.param_points(stage)]
        for a, b in zip(again, want):
            assert a.tobytes() == b.tobytes()
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 2. solver
def test_solver_recovers_a_synthetic_calibration(reg):
    """n = 700 (2 x 256 + 188), noise 1e-3, truth chosen (li_init_shapes.solver_problem).  Stages 1 -> 2 -> 3 follow the numpy
    oracle (equal iteration counts, parameters within 1e-8 / 1e-9 as tests/test_gpu_calib.py holds them) and recover the
    truth no worse than twice the oracle's own error - the two differ in summation order only.
    The oracle's measured error, on the CPU: rotation 1.97e-4 rad, b_g 7.0e-5 rad/s, t_d 8.2e-7 s, T_LI 3.3e-5 m,
    acc_bias 9.5e-4 m/s^2, grav_L0 4.9e-4 m/s^2 (4 / 3 / 4 iterations); the GPU's: profiles/li_init_shapes.md."""
    from lidar_imu_init_amd.api import lii_calib_result
    o = S.oracle_solution()
    s1, s2, s3 = o["s1"], o["s2"], o["s3"]
    reg.calib_set_buffers(o["imu"].to_records(), o["lid"].to_records())
    res = lii_calib_result()
    res.R_LI[:] = list(np.eye(3).reshape(-1))
    reg.calib_solve_stage(1, res)
    assert np.allclose(np.array(res.R_LI[:]).reshape(3, 3), s1["R_LI"], atol=1e-8)
    assert res.iterations[0] == s1["iterations"]
    reg.calib_solve_stage(2, res)
    assert np.allclose(np.array(res.R_LI[:]).reshape(3, 3), s2["R_LI"], atol=1e-8)
    assert np.allclose(res.gyro_bias[:], s2["gyro_bias"], atol=1e-9)
    assert abs(res.time_lag_2 - s2["time_lag_2"]) < 1e-9
    assert res.iterations[1] == s2["iterations"]
    reg.calib_solve_stage(3, res)
    assert np.allclose(res.T_LI[:], s3["T_LI"], atol=1e-8)
    assert np.allclose(res.acc_bias[:], s3["acc_bias"], atol=1e-9)
    assert np.allclose(res.grav_L0[:], s3["grav_L0"], atol=1e-8)
    assert res.iterations[2] == s3["iterations"]
    err = S.recovery_errors(o["truth"], res.R_LI[:], res.gyro_bias[:], res.time_lag_2, res.T_LI[:], res.acc_bias[:], res.grav_L0[:])
    print("recovery error, GPU:", err, "oracle:", o["err"])
    for key, e in err.items():
        assert e <= 2.0 * o["err"][key], key


# ------------------------------------------------------------------------------------------------ 3. zero-phase filter
@pytest.mark.parametrize("n_seq,n", S.ZERO_PHASE_CASES)
def test_zero_phase_batches(reg, n_seq, n):
    from oracle import li_init_np as LI
    batch = S.filter_batch(n_seq, n)
    keep = batch.copy()
    got = reg.zero_phase_filter(batch)
    assert np.array_equal(batch, keep), "the input is not modified"
    for s in range(n_seq):
        want = LI.zero_phase_filt(S.seq_from_records(keep[s])).to_records()
        assert np.array_equal(got[s][:, 9:21], want[:, 9:21]), f"sequence {s}: same additions in the same order, bit-identical"
        assert np.array_equal(got[s][:, :9], keep[s][:, :9]) and np.array_equal(got[s][:, 21], keep[s][:, 21])
        alone = reg.zero_phase_filter(keep[s:s + 1])
        assert alone[0].tobytes() == got[s].tobytes(), f"sequence {s} filtered alone"


def test_zero_phase_rules(reg):
    assert _refused(LII_ERR_INVALID, reg.zero_phase_filter, S.filter_batch(2, 61))
    assert _refused(LII_ERR_INVALID, reg.zero_phase_filter, np.zeros((2, 0, 22)))
    assert _refused(LII_ERR_INVALID, reg.zero_phase_filter, np.zeros((0, 100, 22)))
    b = S.filter_batch(1, 63)
    assert reg.zero_phase_filter(b).tobytes() == reg.zero_phase_filter(b).tobytes()  # the handle stays usable


# ------------------------------------------------------------------------------------------------ 4. cross-correlation
@pytest.mark.parametrize("n,shift", S.ROLLED_CASES)
def test_xcorr_sizes_and_shifts(reg, n, shift):
    from oracle import li_init_np as LI
    a, b = S.rolled_pair(n, shift, seed=4)
    assert reg.xcorr_lag(a.to_records(), b.to_records()) == LI.xcorr_temporal_init(a, b, 50.0)[1]


@pytest.mark.parametrize("k", S.BOUNDARY_K)
def test_xcorr_winner_on_a_stride_boundary(reg, k):
    """n = 300, 599 lags: lanes 0 .. 86 of k_xcorr_argmax hold three lags, the others two; the winner sits at k."""
    from oracle import li_init_np as LI
    n = S.BOUNDARY_N
    a, b = S.windowed_pair(n, k - (n - 1))
    want = LI.xcorr_temporal_init(a, b, 50.0)[1]
    assert (n - 1) - want == k, "the oracle's winner is the intended index"
    assert reg.xcorr_lag(a.to_records(), b.to_records()) == want


def test_xcorr_plateaus(reg):
    from oracle import li_init_np as LI
    n = S.BOUNDARY_N
    a, b = S.plateau_pair()  # every correlation is zero: 599 equal values, the first lag in ascending order wins
    assert np.all(np.linalg.norm(b.ang_vel, axis=1) == 5.0)
    for x, y in ((a, b), (b, a)):
        want = LI.xcorr_temporal_init(x, y, 50.0)[1]
        assert want == n - 1
        assert reg.xcorr_lag(x.to_records(), y.to_records()) == want
    a, b = S.plateau_pair(peak=True)  # 298 lags tie at exactly 0 under a unique positive peak (asserted on the CPU)
    for x, y in ((a, b), (b, a)):
        assert reg.xcorr_lag(x.to_records(), y.to_records()) == LI.xcorr_temporal_init(x, y, 50.0)[1]
    assert _refused(LII_ERR_INVALID, reg.xcorr_lag, np.zeros((0, 22)), np.zeros((0, 22)))


# ------------------------------------------------------------------------------------------------ 5. lii_li_init_run
def _run_both(reg, imu22, lid22, freq, cut):
    import lidar_imu_init_amd as lii
    out = []
    for on in (False, True):
        reg.li_init_set_device(on)
        try:
            res, lag1, total = reg.li_init_run(imu22, lid22, freq, cut)
            fields = [np.array(getattr(res, f)[:]) for f in ("R_LI", "T_LI", "gyro_bias", "acc_bias", "grav_L0", "final_cost")]
            out.append((0, b"".join(x.tobytes() for x in fields) + np.array([res.time_lag_2, lag1, total]).tobytes(), lag1))
        except lii.LIIError as e:
            out.append((e.code, b"", None))
        finally:
            reg.li_init_set_device(False)
    return out


@pytest.mark.parametrize("n_states", (400, 900))
def test_li_init_run_device_chain_equals_host_chain(reg, n_states):
    imu22, lid22 = S.synthetic_accumulation(n_states)
    assert abs(len(imu22) - n_states) < 30 and len(imu22) != 1369
    host, dev = _run_both(reg, imu22, lid22, 20, 1)
    assert host[0] == 0 and dev[0] == 0
    assert host[1] == dev[1], "R_LI, T_LI, gyro_bias, acc_bias, grav_L0, final_cost, both lags and the total: bit-identical"


def test_li_init_run_short_sequences_fall_back_to_the_host_chain(reg):
    """A cross-correlation lag of 108 samples leaves 61 states for the second zero-phase filter: under the device filter's 62,
    so the switched-on run takes the host filter there (after the device's first filter and cross-correlation) and must return
    what the host chain returns.  With 58 states left the host filter's 60-sample reflection would read outside the sequence:
    both chains refuse."""
    imu, lid = S.short_accumulation(108)
    host, dev = _run_both(reg, imu.to_records(), lid.to_records(), 10, 5)
    assert host[0] == 0 and dev[0] == 0 and host[1] == dev[1]
    assert host[2] == -108 / 50.0
    imu, lid = S.short_accumulation(112)
    host, dev = _run_both(reg, imu.to_records(), lid.to_records(), 10, 5)
    assert host[0] == LII_ERR_INVALID and dev[0] == LII_ERR_INVALID
    imu22, lid22 = S.short_accumulation(108)[0].to_records(), S.short_accumulation(108)[1].to_records()
    assert _run_both(reg, imu22, lid22, 10, 5)[0][0] == 0  # the handle stays usable after the refusal
