"""The scan front end - the de-skew launch (k_deskew_imu / _dev / _gated / k_deskew_cv / _cv_prop, lii_scan.hip) and the hashed voxel
filter behind it (vhash_insert_abs / k_vhash_insert, k_vhash_emit) - must give THE SAME BITS as the library that recorded
tests/golden/front_end_bits/cases.npz (tools/record_front_end_bits.py; recorded with the commit before the insert moved in front of
the bounding box, the box reduction went to DPP row operations, the head search went to one ballot per wavefront and the emit
published its count before it folds the box).  All of that re-schedules work and keeps every float operation, the points, their order
and the centroids as they were, so nothing is tolerated: np.array_equal on the de-skewed scan (scan_download(0)), the down-sampled
cloud in the reference's order (scan_download(1): the library's pcl_out order), n_down, and - for the calls that register - the final
lii_state, normal_eq, iterations and effect_num.  The order of the cloud ON THE DEVICE is not downloadable; it decides which points share
a partial sum of the fit launch, so the recorded state and normal_eq hold it.

The library is not only compared with itself: every case's de-skewed scan is held to oracle.undistort_imu / oracle.undistort_cv
(<= 2 float ulp per coordinate, stamps equal: tests/test_gpu_scan_ops.py) and every case's down-sampled cloud to
oracle.voxel_grid of the de-skewed scan (bit for bit, in the reference's order).

Cases (small on purpose; run_cases lists them):
  sizes       1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1 023, 1 025, 5 000 points of a `vlp16` scan (tiny: the 2 048-point one),
              thinned evenly so that every size spans the whole sweep: one lane, the seams of a wavefront, of a workgroup and of a
              grid of two points per lane, several workgroups (prefix_below has lower blocks)
  pose tables K = 2, 12, 29 (the pre-armed form's largest), 30 (the plain form), 64 (kernel arguments), 65 (device table); every
              point under one head; every full wavefront across two heads; a point whose time equals a pose time (strict >)
  order       time-sorted (scan_sorted = 1), as the sensor model emits it (0), sorted on the device (2)
  points      first point under several heads (quirk A3); NaN / +-inf at the first, a middle and the last index; all points in one
              voxel (more than kVhMembers = 10 members), 40 of 513 in one voxel; every point alone; coordinates on voxel faces on both
              sides of zero and -0.0f (under a table that moves no point); a leaf the overflow guard refuses; leaf 0
  paths       lii_scan_register plain and announced (pre-armed), lii_scan_register_cv, lii_undistort_imu / _cv + lii_downsample,
              LII_TEST = no_fuse, no_fast, emit_late"""
import os

import numpy as np
import pytest

from conftest import make_state

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "front_end_bits", "cases.npz")
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025, 5000)
LEAF, MAX_IT = 0.1, 3
R_LI = (0.01, 0.02, -0.015)
T_LI = (0.03, -0.02, 0.05)


def _ulp_diff(a, b):  # tests/test_gpu_scan_ops.py
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


class World:
    """The scans, the start state and the pose tables every case is cut from (built once)."""

    def __init__(self, oracle, small_world):
        import lidar_imu_init_amd as lii
        from harness import synth
        self.O, self.lii, self.synth = oracle, lii, synth
        self.hall, self.map_pts = small_world
        self.R = synth.rot_zyx(0.03, -0.02, 0.4)
        self.p = np.array([0.8, -0.6, 0.1])
        self.R_LI = synth.rot_zyx(*R_LI)
        self.T_LI = np.array(T_LI)
        Rw = self.R @ self.R_LI.T  # (the scan is taken from the LiDAR's pose: test_gpu_solve_bits.py)
        self.Rw, self.pw = Rw, self.p - Rw @ self.T_LI
        st_true = make_state(oracle, self.Rw, self.pw, self.R_LI, self.T_LI)
        self.st0 = lii.State(oracle.state_boxplus(st_true, np.r_[0.004, -0.003, 0.005, 0.03, -0.02, 0.01, np.zeros(18)]))
        self.st_cv = self.st0.copy()  # (CV model: bias_g = omega, vel_end = v)
        self.st_cv.bias_g[:] = [0.04, -0.03, 0.09]
        self.st_cv.vel_end[:] = [0.3, -0.1, 0.02]
        self.raw = {s: synth.make_scan(self.hall, s, self.R, self.p, noise=0.02, seed=11) for s in ("vlp16", "tiny")}

    def scan(self, n, sorted_=True, sensor="vlp16"):
        """n points of the sweep, thinned evenly; sorted_: in ascending time order (stable), else in the sensor model's ring order."""
        raw = self.raw[sensor]
        pts = raw[np.linspace(0, len(raw) - 1, n).astype(np.int64)] if n > 1 else raw[len(raw) // 2:len(raw) // 2 + 1]
        if sorted_:
            pts = pts[np.argsort(pts[:, 3], kind="stable")]
        return np.ascontiguousarray(pts, np.float32)

    def table(self, K=None, times=None, seed=1):
        """A pose table around the state's end pose: gentle motion, so that the registration behind it stays a registration."""
        rng = np.random.default_rng(seed)
        if times is None:
            times = np.r_[0.0, np.sort(rng.uniform(0.002, 0.1, K - 1))]
        T = self.lii.pose6d_array(len(times))
        for k, t in enumerate(times):
            T[k, 0] = t
            T[k, 1:4] = rng.normal(0, 0.3, 3)
            T[k, 4:7] = rng.normal(0, 0.2, 3)
            T[k, 7:10] = rng.normal(0, 0.2, 3)
            T[k, 10:13] = self.st0.pos_end + rng.normal(0, 0.01, 3)
            T[k, 13:22] = (self.st0.rot_end @ self.synth.rot_zyx(*rng.normal(0, 0.005, 3))).reshape(-1)
        return T


def _downloads(reg, leaf):
    out = dict(deskewed=reg.scan_download(0).copy())
    try:
        out["down"] = reg.scan_download(1).copy()
    except Exception as e:  # (no down-sampled cloud: the call before failed)
        out["down"] = np.zeros((0, 4), np.float32)
        out["down_error"] = np.int64(getattr(e, "code", -1))
    out["n_down"] = np.int64(len(out["down"]))
    return out


def _registered(reg, call):
    """The record of a registering call: the report and the state, or the error code it failed with (a cloud of a handful of points
    is no registration - the front end ran all the same and is recorded)."""
    try:
        st, rep = call()
        return dict(state=st.pod.copy(), normal_eq=np.array(rep["normal_eq"], np.float64), iterations=np.int64(rep["iterations"]),
                    effect_num=np.int64(rep["effect_num"]), error=np.int64(0))
    except Exception as e:
        return dict(state=np.zeros(0), normal_eq=np.zeros(0), iterations=np.int64(-1), effect_num=np.int64(-1), error=np.int64(getattr(e, "code", -1)))


def _plain(w, reg, pts, T, leaf=LEAF, sorted_=True, st=None):
    reg.scan_upload(pts)

    def call():
        s = (st or w.st0).copy()
        return s, reg.scan_register(s, st or w.st0, imu_poses=T, leaf=leaf, max_iterations=MAX_IT, imu_en=True, scan_sorted=sorted_)
    out = _registered(reg, call)
    out.update(_downloads(reg, leaf))
    return out


def _announced(w, reg, pts, T, leaf=LEAF):
    """The same scan twice from a caller's device buffer, the first call announcing the second: the second call's prologue is the pre-armed one."""
    dev = reg.device_scan(pts)
    out = None
    for k in range(2):
        def call():
            s = w.st0.copy()
            return s, reg.scan_register(s, w.st0, imu_poses=T, leaf=leaf, max_iterations=MAX_IT, imu_en=True, scan_dev=dev, scan_sorted=True,
                                        next_scan=dev if k == 0 else None)
        out = _registered(reg, call)
    out.update(_downloads(reg, leaf))
    return out


def _cv(w, reg, pts, leaf=LEAF, sorted_=True):
    reg.scan_upload(pts)

    end = {}

    def call():
        s, prop, rep = reg.register_cv(0.1, 0.01, 0.01, w.st_cv.copy(), leaf=leaf, max_iterations=MAX_IT, scan_sorted=sorted_)
        end["rot"] = prop.rot_end.copy()  # (rot_end * Exp(bias_g, dt), formed on the device: the rotation the scan's workgroups de-skew to)
        return s, rep
    out = _registered(reg, call)
    out["end_rot"] = end["rot"]
    out.update(_downloads(reg, leaf))
    return out


def _separate(w, reg, pts, T, leaf=LEAF, cv=False):
    reg.scan_upload(pts)
    if cv:
        reg.undistort_cv(w.st_cv.bias_g, w.st_cv.vel_end, w.st_cv.rot_end)
    else:
        reg.undistort_imu(T, w.st0.rot_end, w.st0.pos_end, w.st0.offset_R_L_I, w.st0.offset_T_L_I)
    if leaf > 0:
        reg.downsample(leaf)
    else:
        reg.downsample_skip()
    return _downloads(reg, leaf)


def _with_env(value, fn):
    old = os.environ.get("LII_TEST")
    if value is None:
        os.environ.pop("LII_TEST", None)
    else:
        os.environ["LII_TEST"] = value
    try:
        return fn()
    finally:
        os.environ.pop("LII_TEST", None)
        if old is not None:
            os.environ["LII_TEST"] = old


def run_cases(oracle, small_world):
    """Every case's result with the library that is loaded: ({name: {field: array}}, {name: inputs for the oracle checks}).  The
    recorder and the test share it."""
    w = World(oracle, small_world)
    lii = w.lii
    out, inputs = {}, {}

    def put(name, res, pts, T=None, cv=False, leaf=LEAF, sorted_=True):
        out[name] = res
        inputs[name] = dict(pts=pts, T=T, cv=cv, leaf=leaf, sorted=sorted_)

    def registrar():
        reg = lii.Registrar(max_scan_points=8_000, max_map_points=400_000, filter_size_map=0.15)
        reg.map_build(w.map_pts)
        return reg

    T12 = w.table(12)
    reg = registrar()
    try:
        # ---- sizes: the fused launch (sorted scan, table in the kernel arguments), the separate calls, and the CV form
        for n in SIZES:
            pts = w.scan(n)
            put(f"plain_n{n}", _plain(w, reg, pts, T12), pts, T12)
            put(f"separate_n{n}", _separate(w, reg, pts, T12), pts, T12)
        for n in (1, 2, 65, 257, 513, 1025):
            pts = w.scan(n)
            put(f"cv_n{n}", _cv(w, reg, pts), pts, cv=True)
        for n in (65, 1025):
            pts = w.scan(n)
            put(f"separate_cv_n{n}", _separate(w, reg, pts, None, cv=True), pts, cv=True)
        # ---- the pre-armed prologue
        for n in (1, 257, 1025, 5000):
            pts = w.scan(n)
            put(f"announced_n{n}", _announced(w, reg, pts, T12), pts, T12)
        # ---- pose tables (513 points: eight full wavefronts and one lane)
        pts = w.scan(513)
        for K in (2, 29, 30, 64, 65):
            T = w.table(K, seed=K)
            put(f"plain_K{K}", _plain(w, reg, pts, T), pts, T)
        T29 = w.table(29, seed=29)
        put("announced_K29", _announced(w, reg, pts, T29), pts, T29)
        put("separate_K65", _separate(w, reg, pts, w.table(65, seed=65)), pts, w.table(65, seed=65))
        one_head = w.table(times=np.r_[-1.0, np.linspace(0.2, 0.3, 11)], seed=3)  # every point later than pose 0 alone
        put("plain_one_head", _plain(w, reg, pts, one_head), pts, one_head)
        put("announced_one_head", _announced(w, reg, pts, one_head), pts, one_head)
        t_s = pts[:, 3].astype(np.float64) / 1000.0
        mids = np.arange(32, 512, 64)  # a pose time between lanes 31 and 32 of every full wavefront
        straddle = w.table(times=np.r_[-1.0, 0.5 * (t_s[mids - 1] + t_s[mids]), 0.2], seed=4)
        assert len(straddle) <= 29 and np.all(np.diff(straddle[:, 0]) > 0)
        put("plain_straddle", _plain(w, reg, pts, straddle), pts, straddle)
        put("announced_straddle", _announced(w, reg, pts, straddle), pts, straddle)
        put("separate_straddle", _separate(w, reg, pts, straddle), pts, straddle)
        equal = w.table(times=np.r_[0.0, t_s[[100, 255, 256, 400]], 0.2], seed=5)  # t == offset_time: the point stays with the head before
        put("plain_equal_time", _plain(w, reg, pts, equal), pts, equal)
        put("announced_equal_time", _announced(w, reg, pts, equal), pts, equal)
        # ---- scan order
        for n in (257, 1025):
            raw = w.scan(n, sorted_=False)
            put(f"plain_unsorted_n{n}", _plain(w, reg, raw, T12, sorted_=False), raw, T12, sorted_=False)
            put(f"plain_devsort_n{n}", _plain(w, reg, raw, T12, sorted_=2), raw, T12, sorted_=2)
            put(f"cv_unsorted_n{n}", _cv(w, reg, raw, sorted_=False), raw, cv=True, sorted_=False)
        raw = w.scan(1025, sorted_=False)
        put("separate_unsorted", _separate(w, reg, raw, T12), raw, T12, sorted_=False)
        put("plain_unsorted_K65", _plain(w, reg, raw, w.table(65, seed=65), sorted_=False), raw, w.table(65, seed=65), sorted_=False)
        # ---- points
        a3 = w.scan(513)
        a3[:, 3] += np.float32(30.0)  # the first point lies behind several pose times: compensated once per head (quirk A3)
        put("plain_a3", _plain(w, reg, a3, T12), a3, T12)
        put("announced_a3", _announced(w, reg, a3, T12), a3, T12)
        put("separate_a3", _separate(w, reg, a3, T12), a3, T12)
        bad = w.scan(513)
        bad[0, 0], bad[256, 1], bad[300, 2], bad[512, 2] = np.nan, np.inf, np.nan, -np.inf
        put("plain_nonfinite", _plain(w, reg, bad, T12), bad, T12)
        put("cv_nonfinite", _cv(w, reg, bad), bad, cv=True)
        put("separate_nonfinite", _separate(w, reg, bad, T12), bad, T12)
        rng = np.random.default_rng(9)
        one = w.scan(65)
        one[:, :3] = (np.float32([5.03, 3.04, 1.05]) + rng.uniform(0, 0.02, (65, 3))).astype(np.float32)
        put("plain_one_voxel", _plain(w, reg, one, T12, leaf=0.5), one, T12, leaf=0.5)
        put("separate_one_voxel", _separate(w, reg, one, T12, leaf=0.5), one, T12, leaf=0.5)
        crowd = w.scan(513)
        at = np.arange(7, 513, 12)[:40]
        crowd[at, :3] = (np.float32([5.03, 3.04, 1.05]) + rng.uniform(0, 0.004, (40, 3))).astype(np.float32)
        put("plain_crowded_voxel", _plain(w, reg, crowd, T12), crowd, T12)
        put("cv_crowded_voxel", _cv(w, reg, crowd), crowd, cv=True)
        pts = w.scan(513)
        put("plain_alone", _plain(w, reg, pts, T12, leaf=0.02), pts, T12, leaf=0.02)
        put("plain_overflow_guard", _plain(w, reg, pts, T12, leaf=0.005), pts, T12, leaf=0.005)
        put("cv_overflow_guard", _cv(w, reg, pts, leaf=0.005), pts, cv=True, leaf=0.005)
        put("separate_overflow_guard", _separate(w, reg, pts, T12, leaf=0.005), pts, T12, leaf=0.005)
        put("plain_leaf0", _plain(w, reg, pts, T12, leaf=0.0), pts, T12, leaf=0.0)
        put("cv_leaf0", _cv(w, reg, pts, leaf=0.0), pts, cv=True, leaf=0.0)
        still = w.table(times=np.linspace(1.0, 1.1, 12), seed=6)  # no point lies behind a pose time: nothing moves
        faces = w.scan(513)
        k = np.arange(-20, 20, dtype=np.float32)
        leaf32 = np.float32(LEAF)
        faces[100:140, 0] = k * leaf32
        faces[140:180, 1] = -k * leaf32
        faces[180:220, 2] = (k / np.float32(8)) * leaf32
        faces[220:230, :3] = np.float32([[-0.0, 0.0, -0.0]])
        faces[230:240, :3] = np.float32([[0.0, -0.0, 0.0]])
        faces[240:250, :3] = np.float32([[-leaf32, leaf32, -0.0]])
        put("plain_faces", _plain(w, reg, faces, still), faces, still)
        put("separate_faces", _separate(w, reg, faces, still), faces, still)
    finally:
        reg.close()
    # ---- the library's test switches, each with a handle of its own (read when the handle is created)
    for env in ("no_fuse", "no_fast", "emit_late"):
        def run():
            r = registrar()
            try:
                for n in (257, 1025, 5000):
                    pts = w.scan(n)
                    put(f"{env}_plain_n{n}", _plain(w, r, pts, T12), pts, T12)
                    if n < 5000:
                        put(f"{env}_cv_n{n}", _cv(w, r, pts), pts, cv=True)
                pts = w.scan(1025)
                put(f"{env}_announced", _announced(w, r, pts, T12), pts, T12)
                put(f"{env}_separate", _separate(w, r, pts, T12), pts, T12)
                raw = w.scan(1025, sorted_=False)
                put(f"{env}_unsorted", _plain(w, r, raw, T12, sorted_=False), raw, T12, sorted_=False)
            finally:
                r.close()
        _with_env(env, run)
    return out, inputs, w


def flatten(got):
    return {f"{name}/{f}": np.asarray(v) for name, case in got.items() for f, v in case.items()}


def load_golden(path=GOLDEN):
    """cases.npz keeps every distinct array once (the paths agree on most of them): `index` maps case/field to its blob."""
    with np.load(path) as z:
        names, at = z["index_names"], z["index_blob"]
        return {str(n): z[f"blob{int(b)}"] for n, b in zip(names, at)}


@pytest.fixture(scope="module")
def ran(oracle, small_world):
    return run_cases(oracle, small_world)


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def test_every_recorded_case_is_run(ran, golden):
    got = flatten(ran[0])
    assert sorted(golden) == sorted(got)
    assert len(ran[0]) >= 90


def test_same_bits_as_the_recorded_library(ran, golden):
    got = flatten(ran[0])
    # (bytes: a NaN coordinate that passes through must come back as the same NaN)
    wrong = [k for k in sorted(got) if not (got[k].shape == golden[k].shape and got[k].dtype == golden[k].dtype and got[k].tobytes() == golden[k].tobytes())]
    for k in wrong:
        print("differs:", k, got[k].shape, golden[k].shape)
    assert not wrong, wrong[:10]


def test_the_cases_take_the_paths_they_are_named_for(ran):
    got = ran[0]
    for n in SIZES:
        if n >= 255:
            assert got[f"plain_n{n}"]["error"] == 0 and got[f"plain_n{n}"]["effect_num"] > 50, n
        assert len(got[f"plain_n{n}"]["deskewed"]) == n
    assert got["plain_overflow_guard"]["n_down"] == 513 and got["plain_leaf0"]["n_down"] == 513  # unfiltered
    assert got["plain_alone"]["n_down"] > 500
    assert got["separate_one_voxel"]["n_down"] == 1
    assert got["plain_nonfinite"]["n_down"] <= 513 - 4
    assert got["plain_crowded_voxel"]["n_down"] < got["plain_n513"]["n_down"]
    # the same scan through every path: the same de-skewed bits and the same cloud
    for a, b in (("plain_n1025", "separate_n1025"), ("plain_n1025", "announced_n1025"), ("plain_n1025", "emit_late_plain_n1025"),
                 ("plain_n1025", "no_fuse_plain_n1025"), ("plain_n1025", "no_fast_plain_n1025"), ("plain_n5000", "announced_n5000"),
                 ("plain_straddle", "announced_straddle"), ("plain_a3", "announced_a3"), ("cv_n1025", "emit_late_cv_n1025"),
                 ("cv_n1025", "no_fuse_cv_n1025"), ("cv_n1025", "no_fast_cv_n1025")):
        assert got[a]["deskewed"].tobytes() == got[b]["deskewed"].tobytes(), (a, b)
        assert got[a]["down"].tobytes() == got[b]["down"].tobytes(), (a, b)
    for a, b in (("plain_n1025", "announced_n1025"), ("plain_n1025", "emit_late_plain_n1025"), ("plain_n5000", "announced_n5000")):
        assert np.array_equal(got[a]["state"], got[b]["state"]) and np.array_equal(got[a]["normal_eq"], got[b]["normal_eq"]), (a, b)


def test_the_front_end_agrees_with_the_oracle(ran):
    """De-skew <= 2 float ulp against the oracle's restatement of the reference (stamps equal, input order kept), centroids bit for bit
    against the oracle's PCL VoxelGrid of the library's own de-skewed scan, in the reference's order."""
    got, inputs, w = ran
    O = w.O
    worst = 0
    for name in sorted(got):
        c, i = got[name], inputs[name]
        pts = i["pts"]
        order = np.argsort(np.where(pts[:, 3] == 0, np.float32(0), pts[:, 3]), kind="stable")  # (the oracle sorts by time, stable; -0.0 == 0.0)
        if i["cv"]:
            ref = O.undistort_cv(pts, w.st_cv.bias_g, w.st_cv.vel_end, c.get("end_rot", w.st_cv.rot_end))  # (lii_scan_register_cv: the propagated end rotation)
        else:
            ref = O.undistort_imu(pts, i["T"], w.st0.rot_end, w.st0.pos_end, w.st0.offset_R_L_I, w.st0.offset_T_L_I)
        d = c["deskewed"] if i["sorted"] != 2 else None
        if d is None:  # sorted on the device: the scan comes back in time order
            d, order = c["deskewed"], np.arange(len(pts))
        assert np.array_equal(d[order, 3], ref[:, 3]), name
        fin = np.isfinite(ref[:, :3]).all(1) & np.isfinite(d[order, :3]).all(1)
        assert np.array_equal(np.isfinite(ref[:, :3]), np.isfinite(d[order, :3])), name
        ulp = int(_ulp_diff(d[order][fin, :3], ref[fin, :3]).max()) if fin.any() else 0
        worst = max(worst, ulp)
        assert ulp <= 2, (name, ulp)
        if i["leaf"] > 0:
            vref, filtered = O.voxel_grid(c["deskewed"], i["leaf"])
            assert c["n_down"] == len(vref), (name, int(c["n_down"]), len(vref))
            assert c["down"].tobytes() == vref.tobytes(), name
        else:
            assert c["down"].tobytes() == c["deskewed"].tobytes(), name
    print("largest de-skew difference against the oracle:", worst, "ulp over", len(got), "cases")
