"""LI-Init on K windows of one accumulation in one call (lii_li_init_windows, lii_li_init_resident.hip): every record against
lii_li_init_resident on the window's slice, run on a second handle, bit for bit; against the numpy oracle (oracle/li_init_np.py)
within the TOL table of tests/test_gpu_li_init_resident.py, unchanged.

Inputs.
  A  synthetic_accumulation(900) (aligned form, orig_odom_freq 20, cut_frame_num 1) with the 200 rows of short_accumulation(112)
     appended.  short_accumulation stamps its rows at 50 Hz, for a job of orig_odom_freq * cut_frame_num = 50; A's job says 20, so
     the appended rows' stamps are re-timed to 20 Hz (the filters and the cross-correlation never read a stamp): the lag of -111
     samples then compensates 111 states away and 58 are left for the second filter, which is the refusal this input exists for.
     With the 50 Hz stamps the same lag is 5.55 s, longer than the 4 s the rows span, and the alignment finds no overlap instead.
  B  the raw accumulation of 900 LiDAR / 9 200 IMU states (_raw_accumulation(900) of tests/test_gpu_li_init_resident.py),
     move_start_time 2.5.
The single call's records are computed once per process and left unchanged; so are the oracle's results."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import li_init_shapes as S  # noqa: E402
import test_gpu_li_init_resident as T  # noqa: E402  (its TOL table and its raw accumulation, as they are)

pytestmark = pytest.mark.gpu

LII_ERR_INVALID, LII_ERR_CAPACITY, LII_ERR_STATE = -1, -4, -5
WIN_OK, WIN_FILTER61, WIN_ALIGNED200 = 0, 1, 2
TOL = T.TOL
assert TOL == dict(R_LI=1e-8, gyro_bias=1e-9, time_lag_2=1e-9, total=1e-9, T_LI=1e-7, acc_bias=1e-8, grav_L0=1e-7)
FREQ, CUT = 20, 1
# (begin, count): the admitted minimum, both sides of a 256-lane workgroup and of a 512 boundary, offset starts, overlaps
ALIGNED = ((0, 200), (0, 201), (0, 256), (0, 257), (0, 400), (0, 900), (300, 300), (700, 200), (100, 513))
SHORT = (900, 200)
# (imu_begin, imu_count, lidar_begin, lidar_count, move_start_time); the fourth starts inside both sequences, the last is refused
RAW = ((0, 2497, 0, 230, 2.5), (0, 4697, 0, 450, 2.5), (0, 9197, 0, 900, 2.5), (2010, 3180, 200, 300, 10.0), (0, 1697, 0, 150, 2.5))


def _registrar():
    import lidar_imu_init_amd as lii
    return lii.Registrar(max_scan_points=1000, max_map_points=1000)


@pytest.fixture(scope="module")
def reg():
    r = _registrar()
    yield r
    r.close()


@pytest.fixture(scope="module")
def single():
    """the second handle: lii_li_init_resident on slices"""
    r = _registrar()
    yield r
    r.close()


_cache = {}


def _A():
    if "A" not in _cache:
        imu, lid = S.synthetic_accumulation(900)
        assert len(imu) == len(lid) == 900
        si, sl = S.short_accumulation(112)
        si, sl = si.to_records(), sl.to_records()
        for rows in (si, sl):
            rows[:, 21] = 100.0 + (rows[:, 21] - 10.0) * 2.5  # 50 Hz -> 20 Hz, behind A's last stamp (module docstring)
        _cache["A"] = (np.ascontiguousarray(np.vstack([imu, si])), np.ascontiguousarray(np.vstack([lid, sl])))
    return _cache["A"]


def _B():
    if "B" not in _cache:
        imu_all, lid, mst = T._raw_accumulation(900)
        assert (len(lid), len(imu_all), mst) == (900, 9200, 2.5)
        _cache["B"] = (np.ascontiguousarray(imu_all), np.ascontiguousarray(lid))
    return _cache["B"]


def _rec_bytes(q):
    """everything of a record but launches / host_waits: status, the result's bytes, the report's lags, counts, terminations, params"""
    rep = q.rep
    return (q.status, bytes(q.res), rep.struct_size, rep.n_aligned, rep.n_stage12, rep.n_stage3, rep.lag_samples, tuple(rep.termination[:]),
            np.float64(rep.time_lag_1).tobytes(), np.float64(rep.total_time_lag).tobytes(), bytes(rep.params))


def _single_bytes(res, rep):
    return (WIN_OK, bytes(res), rep.struct_size, rep.n_aligned, rep.n_stage12, rep.n_stage3, rep.lag_samples, tuple(rep.termination[:]),
            np.float64(rep.time_lag_1).tobytes(), np.float64(rep.total_time_lag).tobytes(), bytes(rep.params))


def _single_aligned(single, w):
    """lii_li_init_resident on the slice of A, once per window"""
    key = ("single", w)
    if key not in _cache:
        imu, lid = _A()
        b, c = w
        _cache[key] = _single_bytes(*single.li_init_resident(imu[b:b + c], lid[b:b + c], FREQ, CUT))
    return _cache[key]


def _single_raw(single, w):
    key = ("single_raw", w)
    if key not in _cache:
        imu, lid = _B()
        ib, ic, lb, lc, mst = w
        _cache[key] = _single_bytes(*single.li_init_resident(imu[ib:ib + ic], lid[lb:lb + lc], FREQ, CUT, interpolate=True, move_start_time=mst))
    return _cache[key]


def _windows_aligned(reg, wins):
    imu, lid = _A()
    return reg.li_init_windows_records(imu, lid, wins, FREQ, CUT)


def _oracle(key):
    if ("oracle", key) not in _cache:
        from oracle import li_init_np as LI
        if key[0] == "A":
            imu, lid = _A()
            b, c = key[1]
            si, sl = S.seq_from_records(imu[b:b + c]), S.seq_from_records(lid[b:b + c])
        else:
            imu, lid = _B()
            ib, ic, lb, lc, mst = key[1]
            si, sl = LI.downsample_interpolate_imu(S.seq_from_records(imu[ib:ib + ic]), S.seq_from_records(lid[lb:lb + lc]), mst)
        out = LI.li_initialization(si, sl, FREQ, CUT)
        out["n_aligned"] = len(si)
        _cache[("oracle", key)] = out
    return _cache[("oracle", key)]


# ------------------------------------------------------------------------------------------------ 1. the single call's bits
def test_each_record_is_the_single_calls(reg, single):
    out = _windows_aligned(reg, ALIGNED)
    for w, q in zip(ALIGNED, out):
        want = _single_aligned(single, w)
        got = _rec_bytes(q)
        print(f"window {w}: status {q.status} iterations {q.res.iterations[:]} n12 {q.rep.n_stage12} n3 {q.rep.n_stage3} lag {q.rep.lag_samples} "
              f"equal bits: {got == want}")
        assert got == want, w


# ------------------------------------------------------------------------------------------------ 2. no dependence on the batch
def test_a_record_does_not_depend_on_the_batch(reg):
    alone = {w: _rec_bytes(_windows_aligned(reg, [w])[0]) for w in ALIGNED}
    forms = dict(together=list(ALIGNED), reversed=list(reversed(ALIGNED)), doubled=[w for w in ALIGNED for _ in (0, 1)],
                 second_call=list(ALIGNED), cyclic_257=[ALIGNED[k % len(ALIGNED)] for k in range(257)])
    for name, wins in forms.items():
        out = _windows_aligned(reg, wins)
        bad = [(k, w) for k, (w, q) in enumerate(zip(wins, out)) if _rec_bytes(q) != alone[w]]
        print(f"{name}: {len(wins)} windows, {len(bad)} differ from the window alone")
        assert not bad, (name, bad[:4])


# ------------------------------------------------------------------------------------------------ 3. a refused window
def test_refused_window_leaves_the_others_alone(reg, single):
    from oracle import li_init_np as LI
    imu, lid = _A()
    b, c = SHORT
    si, sl = S.seq_from_records(imu[b:b + c]), S.seq_from_records(lid[b:b + c])
    # the oracle's chain up to the second filter (li_initialization, oracle/li_init_np.py): 58 states are left
    i0, l0 = LI.imu_time_compensate(si, sl, 0.0, True)
    i1, l1 = LI.normalize_acc(LI.zero_phase_filt(i0)), LI.zero_phase_filt(l0)
    i1, l1 = LI.cut_sequence_tail(i1.slice(slice(0, len(i1) - 1)), l1.slice(slice(0, len(l1) - 1)))
    lag1, _ = LI.xcorr_temporal_init(i1, l1, FREQ * CUT)
    i2, _ = LI.imu_time_compensate(i1, l1, lag1, False)
    assert len(i2) == 58
    wins = [ALIGNED[0], SHORT, ALIGNED[6], SHORT, ALIGNED[5]]
    out = _windows_aligned(reg, wins)  # returns: the call's code is LII_OK
    for w, q in zip(wins, out):
        if w == SHORT:
            assert q.status == WIN_FILTER61
            assert bytes(q)[4:] == bytes(C.sizeof(type(q)) - 4), "everything behind the status is zero"
        else:
            assert _rec_bytes(q) == _single_aligned(single, w), w
    again = _windows_aligned(reg, [ALIGNED[1]])  # the handle serves a further call
    assert _rec_bytes(again[0]) == _single_aligned(single, ALIGNED[1])
    rec = reg.li_init_windows(imu, lid, wins, FREQ, CUT)
    assert list(rec["status"]) == [0, 1, 0, 1, 0] and not rec[1]["R_LI"].any() and rec[0]["n_aligned"] == 200


# ------------------------------------------------------------------------------------------------ 4. the raw form
def test_raw_form(reg, single):
    imu, lid = _B()
    out = reg.li_init_windows_records(imu, lid, RAW, FREQ, CUT, interpolate=True)
    for w, q in zip(RAW[:4], out):
        want = _single_raw(single, w)
        print(f"raw window {w}: status {q.status} n_aligned {q.rep.n_aligned} iterations {q.res.iterations[:]} equal bits: {_rec_bytes(q) == want}")
        assert _rec_bytes(q) == want, w
    assert [q.rep.n_aligned for q in out[:3]] == [230, 450, 900] == [_oracle(("B", w))["n_aligned"] for w in RAW[:3]]
    assert out[4].status == WIN_ALIGNED200 and bytes(out[4])[4:] == bytes(C.sizeof(type(out[4])) - 4)
    # the raw windows in another order, the refused one first
    rev = reg.li_init_windows_records(imu, lid, list(reversed(RAW)), FREQ, CUT, interpolate=True)
    assert [_rec_bytes(q) for q in reversed(rev)] == [_rec_bytes(q) for q in out]


# ------------------------------------------------------------------------------------------------ 5. the oracle
def _check_against_oracle(q, out, who):
    got = dict(R_LI=np.array(q.res.R_LI[:]), gyro_bias=np.array(q.res.gyro_bias[:]), time_lag_2=np.array([q.res.time_lag_2]),
               total=np.array([q.rep.total_time_lag]), T_LI=np.array(q.res.T_LI[:]), acc_bias=np.array(q.res.acc_bias[:]),
               grav_L0=np.array(q.res.grav_L0[:]))
    want = dict(R_LI=out["stage2"]["R_LI"].reshape(-1), gyro_bias=out["stage2"]["gyro_bias"], time_lag_2=np.array([out["stage2"]["time_lag_2"]]),
                total=np.array([out["time_delay"]]), T_LI=out["stage3"]["T_LI"], acc_bias=out["stage3"]["acc_bias"], grav_L0=out["stage3"]["grav_L0"])
    its = [out["stage1"]["iterations"], out["stage2"]["iterations"], out["stage3"]["iterations"]]
    print(f"{who}: iterations {q.res.iterations[:]} oracle {its}; lag {q.rep.lag_samples} oracle {out['lag_frames']}")
    worst = []
    for k in TOL:
        d = np.max(np.abs(got[k] - want[k]))
        print(f"{who} {k}: |windows - oracle| {d:.3e} (tolerance {TOL[k]:.0e})")
        if not d <= TOL[k]:
            worst.append(k)
    assert q.status == WIN_OK
    assert not worst, (who, worst)
    assert q.res.iterations[:] == its and q.rep.lag_samples == out["lag_frames"]


def test_against_the_oracle(reg):
    wins = [(0, 200), (300, 300), (0, 900)]
    for w, q in zip(wins, _windows_aligned(reg, wins)):
        _check_against_oracle(q, _oracle(("A", w)), f"A{w}")
    imu, lid = _B()
    q = reg.li_init_windows_records(imu, lid, [RAW[1]], FREQ, CUT, interpolate=True)[0]
    _check_against_oracle(q, _oracle(("B", RAW[1])), "B 450 states")


# ------------------------------------------------------------------------------------------------ 6. an observer of the handle
def test_the_call_observes_the_calibration_state():
    r = _registrar()
    try:
        imu, lid = _A()
        r.li_init_resident(imu[:400], lid[:400], FREQ, CUT)
        rng = np.random.default_rng(7)
        points = {1: S.pack_params(1, S.rand_rot(rng), np.zeros(0), None),
                  2: S.pack_params(2, S.rand_rot(rng), np.r_[rng.normal(0, 0.01, 3), 0.003], None),
                  3: S.pack_params(3, S.rand_rot(rng), np.r_[rng.normal(0, 0.005, 3), rng.normal(0, 0.2, 3)], S.rand_rot(rng))}

        def state():
            fetched = tuple(a.tobytes() for which in (1, 2) for a in r.li_init_resident_fetch(which))
            return fetched + tuple(S.flat(*r.calib_eval(stage, p)).tobytes() for stage, p in points.items())

        before = state()
        out = r.li_init_windows_records(imu, lid, [(0, 900), (100, 513), SHORT], FREQ, CUT)
        assert [q.status for q in out] == [WIN_OK, WIN_OK, WIN_FILTER61]
        assert state() == before
        bi, bl = _B()
        r.li_init_windows_records(bi, bl, RAW[:1], FREQ, CUT, interpolate=True)
        assert state() == before
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 7. refusals on the host
def test_host_refusals_on_a_live_handle(reg):
    import lidar_imu_init_amd as lii
    from lidar_imu_init_amd import api
    imu, lid = _A()
    n = len(imu)

    def refused(code, wins, **kw):
        with pytest.raises(lii.LIIError) as e:
            reg.li_init_windows_records(imu, lid, wins, FREQ, CUT, **kw)
        assert e.value.code == code, (e.value.code, code, wins)

    refused(LII_ERR_INVALID, [(0, 199)])
    refused(LII_ERR_INVALID, [(n - 199, 200)])                # past the end
    refused(LII_ERR_INVALID, [(0, 400), (-1, 200)])
    refused(LII_ERR_INVALID, [(1, 300, 0, 300)])              # imu_begin != lidar_begin
    refused(LII_ERR_INVALID, [(0, 300, 0, 301)])
    refused(LII_ERR_INVALID, [(0, 5, 0, 300)], interpolate=True)
    refused(LII_ERR_INVALID, [(0, 300, 0, 0)], interpolate=True)
    refused(LII_ERR_INVALID, [])                              # n_windows 0
    refused(LII_ERR_INVALID, [(0, 200)] * 4097)
    job = api.lii_li_init_job(C.sizeof(api.lii_li_init_job), 0, imu.ctypes.data, n, lid.ctypes.data, n, 0.0, FREQ, CUT)
    win = api.li_init_window_array([(0, 200)])
    out = (api.lii_li_init_window_result * 1)()
    size = C.sizeof(api.lii_li_init_window_result)
    call = reg.L.lii_li_init_windows
    assert call(reg.h, C.byref(job), win.ctypes.data, 1, C.addressof(out), size - 8) == LII_ERR_INVALID  # out_stride
    assert call(reg.h, C.byref(job), win.ctypes.data, 1, C.addressof(out), 0) == LII_ERR_INVALID
    assert call(reg.h, C.byref(job), None, 1, C.addressof(out), size) == LII_ERR_INVALID
    assert call(reg.h, C.byref(job), win.ctypes.data, 1, None, size) == LII_ERR_INVALID
    assert call(reg.h, None, win.ctypes.data, 1, C.addressof(out), size) == LII_ERR_INVALID
    job.struct_size = 8
    assert call(reg.h, C.byref(job), win.ctypes.data, 1, C.addressof(out), size) == LII_ERR_INVALID
    job.struct_size = C.sizeof(api.lii_li_init_job)
    # scratch beyond the stated limit: 4096 windows of 900 000 states (the ranges are checked against the job's n alone)
    big = api.lii_li_init_job(C.sizeof(api.lii_li_init_job), 0, imu.ctypes.data, 900_000, lid.ctypes.data, 900_000, 0.0, FREQ, CUT)
    wins = api.li_init_window_array([(0, 900_000)] * 4096)
    outs = (api.lii_li_init_window_result * 4096)()
    assert call(reg.h, C.byref(big), wins.ctypes.data, 4096, C.addressof(outs), size) == LII_ERR_CAPACITY
    assert call(reg.h, C.byref(job), win.ctypes.data, 1, C.addressof(out), size) == 0 and out[0].status == WIN_OK


def test_refused_from_inside_while_waiting():
    """lii_scan_job::while_waiting runs on the host between a registration's launches and its wait: the windows call is refused there
    with LII_ERR_STATE and served again behind the registration."""
    import lidar_imu_init_amd as lii
    from harness import synth
    from lidar_imu_init_amd import api
    from oracle import oracle as O
    imu, lid = _A()
    hall = synth.Hall(size=(20.0, 16.0, 6.0), n_boxes=6, seed=3)
    map_pts = hall.surface_points(0.3, noise=0.01, seed=3)
    scan = synth.make_scan(hall, "tiny", np.eye(3), np.zeros(3), noise=0.02, seed=5)
    r = lii.Registrar(max_scan_points=10_000, max_map_points=max(len(map_pts), 1000), filter_size_map=0.3)
    try:
        r.map_build(map_pts)
        r.scan_upload(scan)
        st = lii.State(O.state_init())
        seen = []

        def hook():
            try:
                r.li_init_windows_records(imu, lid, [(0, 200)], FREQ, CUT)
                seen.append(0)
            except api.LIIError as e:
                seen.append(e.code)

        r.scan_register(st, st.copy(), leaf=0.0, max_iterations=2, while_waiting=hook)
        assert seen == [LII_ERR_STATE]
        assert r.li_init_windows_records(imu, lid, [(0, 200)], FREQ, CUT)[0].status == WIN_OK
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 8. a constant launch sequence
def test_launches_waits_and_allocations():
    r = _registrar()
    try:
        imu, lid = _A()
        assert r.li_init_windows_scratch() == (0, 0)
        big = r.li_init_windows_records(imu, lid, [ALIGNED[k % len(ALIGNED)] for k in range(257)], FREQ, CUT)
        scratch = r.li_init_windows_scratch()
        one = r.li_init_windows_records(imu, lid, [ALIGNED[5]], FREQ, CUT)
        assert big[0].rep.launches == one[0].rep.launches > 0
        assert all(q.rep.launches == big[0].rep.launches and q.rep.host_waits == 1 for q in big) and one[0].rep.host_waits == 1
        r.li_init_windows_records(imu, lid, list(ALIGNED), FREQ, CUT)
        assert r.li_init_windows_scratch() == scratch, "a call no larger than an earlier one allocates nothing"
        print(f"launches {one[0].rep.launches}, scratch for 257 windows of up to 900 states {scratch[0]} bytes in {scratch[1]} allocations")
    finally:
        r.close()
