"""The registered clouds as message bytes (lii_publish_wire_set / _wire_fetch, lii_publish_saved_pcd; lii_publish.hip: the WIRE
instantiations of k_publish_world, k_pcd_rows): the bytes pcl::toROSMsg puts into sensor_msgs/PointCloud2::data for laserCloudWorld /
feats_undistort / laserCloudOri (src/laserMapping.cpp:561-586, :616-623, :625-636) and the rows PCDWriter::writeBinary writes (:609).

Reference: the float4 clouds and intensities of the SAME call (lii_publish_fetch / lii_publish_fetch_intensity, held against the oracle
in tests/test_gpu_publish.py and tests/test_gpu_intensity.py), packed into 48-byte pcl::PointXYZINormal records by numpy here.  Every
comparison is bit for bit (uint32 views), no tolerance.  Worlds: those of tests/test_gpu_publish.py - a hall, a map of a few thousand
points, scans of at most 4 099 points (16 384 for the staging-chunk case), max_scan_points 20 000."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, STATE = -1, -4, -5
DENSE, DOWN, EFFECT, BODY, INTENSITY = 1, 2, 4, 8, 16
ALL = DENSE | DOWN | EFFECT | BODY
MAX_SCAN = 20_000
ONE = 0x3F800000
EFFECT_INTENSITY = np.float32(np.sqrt(np.float64(1000.0)))  # src/laserMapping.cpp:1050-1051
_cache = {}


def _world():
    if "w" not in _cache:
        import lidar_imu_init_amd as lii
        from harness import synth
        hall = synth.Hall(size=(20.0, 16.0, 6.0), n_boxes=6, seed=3)
        map_pts = hall.surface_points(0.4, noise=0.01, seed=3)
        R = synth.rot_zyx(0.02, -0.01, 0.3)
        p = np.array([0.5, -0.4, 0.1])
        scan = synth.make_scan(hall, "mid16k", R, p, noise=0.02, seed=5)
        st = lii.State()
        st.rot_end[:] = R @ synth.rot_zyx(0.004, -0.003, 0.005)
        st.pos_end[:] = p + np.array([0.03, -0.02, 0.02])
        st.offset_R_L_I[:] = synth.rot_zyx(0.01, -0.02, 0.015)
        st.offset_T_L_I[:] = [0.04, -0.02, 0.05]
        st.gravity[:] = [0, 0, -9.81]
        _cache["w"] = dict(hall=hall, map=map_pts, R=R, p=p, scan=scan, st=st)
    return _cache["w"]


def _registrar(env=None, **kw):
    import lidar_imu_init_amd as lii
    w = _world()
    old = os.environ.get("LII_TEST")
    os.environ.pop("LII_TEST", None)
    if env:
        os.environ["LII_TEST"] = env
    try:
        reg = lii.Registrar(**{**dict(max_scan_points=MAX_SCAN, max_map_points=max(4 * len(w["map"]), 50_000), filter_size_map=0.15), **kw})
    finally:
        os.environ.pop("LII_TEST", None)
        if old is not None:
            os.environ["LII_TEST"] = old
    reg.map_build(w["map"])
    return reg


def _poses():
    from harness import synth
    P = np.zeros((3, 22))
    for k, t in enumerate((0.0, 0.05, 0.1)):
        P[k, 0] = t
        P[k, 1:4] = [0.1, -0.05, 0.02]
        P[k, 4:7] = [0.02, -0.01, 0.05]
        P[k, 7:10] = [0.3, -0.2, 0.05]
        P[k, 10:13] = np.array([0.3, -0.2, 0.05]) * t
        P[k, 13:22] = synth.rot_zyx(0.02 * t, -0.01 * t, 0.05 * t).reshape(-1)
    return P


def _take(n, sorted_):
    s = _world()["scan"]
    idx = np.linspace(0, len(s) - 1, n).astype(int) if n > 1 else np.array([len(s) // 2])
    s = s[idx]
    return s[np.argsort(s[:, 3], kind="stable")] if sorted_ else s


def _inten(n, seed):
    """n intensities, none of them zero (a zero word in a record must mean 'not carried')"""
    return np.random.default_rng(seed).uniform(1.0, 255.0, n).astype(np.float32)


def _state(undistort=1):
    st = _world()["st"].copy()
    if undistort == 2:
        st.bias_g[:] = [0.02, -0.01, 0.05]
        st.vel_end[:] = [0.3, -0.2, 0.05]
    return st


def _code(fn):
    import lidar_imu_init_amd as lii
    try:
        fn()
    except lii.LIIError as e:
        return e.code
    return 0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _words(rec):
    """(n, 48) uint8 -> (n, 12) uint32"""
    assert rec.dtype == np.uint8 and rec.ndim == 2 and rec.shape[1] == 48, (rec.dtype, rec.shape)
    return np.ascontiguousarray(rec).view("<u4").reshape(-1, 12)


def _pack(xyz4, intensity, curvature):
    """pcl::PointXYZINormal records by numpy: x y z 1.0f | 0 0 0 0 | intensity curvature 0 0 (all as bit patterns)"""
    n = len(xyz4)
    w = np.zeros((n, 12), np.uint32)
    w[:, 0:3] = _bits(xyz4[:, :3]).reshape(n, 3)
    w[:, 3] = ONE
    w[:, 8] = _bits(np.broadcast_to(np.asarray(intensity, np.float32), (n,))).reshape(n)
    w[:, 9] = _bits(np.broadcast_to(np.asarray(curvature, np.float32), (n,))).reshape(n)
    return w


def _device_rows(dp, n_float4):
    """n float4 of a DEVICE buffer a fetch hands out, read back through a second handle (lii_scan_set_device copies from any device
    pointer, the download returns what it copied): nothing but the library under test touches the device in this process."""
    if "reader" not in _cache:
        import lidar_imu_init_amd as lii
        _cache["reader"] = lii.Registrar(max_scan_points=3 * MAX_SCAN, max_map_points=1000)
    rd = _cache["reader"]
    rd.scan_set_device((dp, n_float4))
    return rd.scan_download(0)


def _fetch_wire(reg, cloud, to_host=True):
    """(n, 12) uint32: the records of one cloud - the pinned copy, or (no to_host) the device buffer"""
    if to_host:
        return _words(reg.publish_wire_fetch(cloud))
    hp, dp, n = C.c_void_p(), C.c_void_p(), C.c_int32(0)
    reg._check(reg.L.lii_publish_wire_fetch(reg.h, int(cloud), C.byref(hp), C.byref(dp), C.byref(n)))
    assert not hp.value and dp.value  # (no host copy was ordered)
    if n.value == 0:
        return np.zeros((0, 12), np.uint32)
    return _device_rows(dp, 3 * n.value).view(np.uint32).reshape(n.value, 12)


def _fetch4(reg, cloud, to_host=True):
    if to_host:
        return reg.publish_fetch(cloud)
    hp, dp, n = C.c_void_p(), C.c_void_p(), C.c_int32(0)
    reg._check(reg.L.lii_publish_fetch(reg.h, int(cloud), C.byref(hp), C.byref(dp), C.byref(n)))
    return _device_rows(dp, n.value) if n.value else np.zeros((0, 4), np.float32)


def _expect(reg, cloud, have_int, to_host=True):
    """The records of `cloud` as the float4 order of the SAME call predicts them."""
    c4 = _fetch4(reg, cloud, to_host)
    if cloud == EFFECT:
        it = EFFECT_INTENSITY
    elif have_int:
        it = reg.publish_fetch_intensity(cloud)
        assert it.shape == (len(c4),)
    else:
        it = np.float32(0.0)
    return _pack(c4, it, c4[:, 3] if cloud == BODY else np.float32(0.0))


def _check_all(reg, have_int, what, to_host=True):
    out = {}
    for cloud in (DENSE, DOWN, EFFECT, BODY):
        got = _fetch_wire(reg, cloud, to_host)
        exp = _expect(reg, cloud, have_int, to_host)
        assert got.shape == exp.shape, (what, cloud, got.shape, exp.shape)
        bad = np.argwhere(got != exp)
        assert len(bad) == 0, (what, cloud, len(bad), bad[:4].tolist())
        out[cloud] = got
    return out


def _register(reg, st, scan, inten, undistort=1, sorted_=True, leaf=0.2, **kw):
    reg.scan_upload(scan)
    if inten is not None:
        reg.scan_intensity_upload(inten)
    form = dict(imu_poses=_poses()) if undistort == 1 else dict(cv=True) if undistort == 2 else {}
    return reg.scan_register(st, st.copy(), leaf=leaf, max_iterations=4, scan_sorted=sorted_, **form, **kw)


def _launches(reg):
    prof, scans = reg.kernel_profile()
    return prof["publish"][1], scans


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
@pytest.mark.parametrize("undistort", [1, 2])
@pytest.mark.parametrize("sorted_", [True, False])
def test_records_of_all_four_clouds(n, undistort, sorted_):
    """Cases 1 and 2 of the feature: both orders on, then the wire order alone on a fresh handle - the same bytes, one launch each."""
    scan, inten = _take(n, sorted_), _inten(n, 100 + n)
    runs = []
    for both in (True, False):
        reg = _registrar()
        if both:
            reg.publish_set(ALL | INTENSITY, to_host=True)
        reg.publish_wire_set(ALL, to_host=True)
        reg.set_profiling(1)
        reg.set_profiling(3)
        st = _state(undistort)
        rep = _register(reg, st, scan, inten, undistort, sorted_)
        if both:
            got = _check_all(reg, True, (n, undistort, sorted_))
            assert len(got[DENSE]) == len(got[BODY]) == n and len(got[EFFECT]) == rep["effect_num"]
            assert len(got[DOWN]) == len(reg.scan_download(1))
            # the time stays where it was: curvature of the world clouds is 0, of the body cloud the cloud's t_ms
            assert not got[DENSE][:, 9].any() and np.array_equal(got[BODY][:, 9], _bits(reg.scan_download(0)[:, 3]))
        else:
            got = {c: _words(reg.publish_wire_fetch(c)) for c in (DENSE, DOWN, EFFECT, BODY)}
            assert _code(lambda: reg.publish_fetch(DENSE)) == STATE  # (the other order is off)
        assert _launches(reg) == (1, 1)  # one publish launch per registration, with either order or both
        runs.append((got, st.pod.copy(), rep["effect_num"]))
        reg.close()
    print(f"n {n} undistort {undistort} sorted {sorted_}: down {len(runs[0][0][DOWN])} effect {runs[0][2]}")
    assert np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    for c in (DENSE, DOWN, EFFECT, BODY):
        assert np.array_equal(runs[0][0][c], runs[1][0][c]), c


@pytest.mark.parametrize("n", [257, 4099])
@pytest.mark.parametrize("to_host", [True, False])
def test_no_intensities_attached(n, to_host):
    reg = _registrar()
    reg.publish_set(ALL, to_host=to_host)
    reg.publish_wire_set(ALL, to_host=to_host)
    st = _state()
    _register(reg, st, _take(n, True), None)
    got = _check_all(reg, False, ("no intensities", n), to_host)
    for c in (DENSE, DOWN, BODY):
        assert not got[c][:, 8].any()
    assert (n < 4099 or len(got[EFFECT]) > 0) and np.all(got[EFFECT][:, 8] == _bits(EFFECT_INTENSITY)[0])
    reg.close()


def _prefix_for_voxels(target, leaf):
    """the shortest prefix of the (time-sorted) scan whose voxel grid at `leaf` holds `target` points (the oracle's filter, on the CPU)"""
    from oracle import oracle as O
    s = _take(len(_world()["scan"]), True)
    lo, hi = 1, len(s)
    while lo < hi:
        mid = (lo + hi) // 2
        if len(O.voxel_grid(s[:mid], leaf)[0]) >= target:
            hi = mid
        else:
            lo = mid + 1
    return s[:lo]


@pytest.mark.parametrize("target", [255, 256, 257, 513])
def test_down_sampled_clouds_at_the_workgroup_seams(target):
    """Compaction base x 48 and the partial last slab: the voxel filter's count around one and two workgroups (no de-skew, so that the
    count is the oracle's), then exactly `target` points without a filter."""
    reg = _registrar()
    reg.publish_set(ALL | INTENSITY, to_host=True)
    reg.publish_wire_set(DOWN | EFFECT, to_host=True)
    scan = _prefix_for_voxels(target, 0.25)
    for k, (s, leaf) in enumerate(((scan, 0.25), (_take(target, True), 0.0))):
        st = _state()
        rep = _register(reg, st, s, _inten(len(s), 7 + k), undistort=0, leaf=leaf)
        down, eff = _words(reg.publish_wire_fetch(DOWN)), _words(reg.publish_wire_fetch(EFFECT))
        print(f"target {target} leaf {leaf}: scan {len(s)} -> down-sampled {len(down)}, effect {len(eff)}")
        assert abs(len(down) - target) <= (2 if leaf else 0) and len(eff) == rep["effect_num"] > 0
        assert np.array_equal(down, _expect(reg, DOWN, True)) and np.array_equal(eff, _expect(reg, EFFECT, True))
        assert _code(lambda: reg.publish_wire_fetch(DENSE)) == STATE  # not ordered as records
    reg.close()


def test_nothing_selected_and_a_start_pose_far_off():
    reg = _registrar()
    reg.publish_set(ALL | INTENSITY, to_host=True)
    reg.publish_wire_set(ALL, to_host=True)
    far = _state()
    far.pos_end[:] += [500.0, 0, 0]
    n = 3000
    reg.scan_upload(_take(n, True))
    reg.scan_intensity_upload(_inten(n, 3))
    rep = reg.scan_register(far, far.copy(), leaf=0.0, max_iterations=3, scan_sorted=True)
    got = _check_all(reg, True, "far off")
    assert rep["effect_num"] == 0 and got[EFFECT].shape == (0, 12) and len(got[DOWN]) == n
    hp, dp, cnt = C.c_void_p(), C.c_void_p(), C.c_int32(-1)
    assert reg.L.lii_publish_wire_fetch(reg.h, EFFECT, C.byref(hp), C.byref(dp), C.byref(cnt)) == 0 and cnt.value == 0
    reg.close()


def test_late_count_words():
    """LII_TEST=emit_late (read when the handle is created, as tests/test_gpu_publish.py sets it): every seventh workgroup of the
    down-sampled cloud hands its count on late - the same records at the same places."""
    scan, inten = _take(8000, True), _inten(8000, 9)  # leaf 0: 32 workgroups
    out = []
    for env in (None, "emit_late"):
        reg = _registrar(env=env)
        reg.publish_set(DOWN | EFFECT | INTENSITY, to_host=True)
        reg.publish_wire_set(DOWN | EFFECT, to_host=True)
        st = _state()
        rep = _register(reg, st, scan, inten, undistort=0, leaf=0.0)
        down, eff = _words(reg.publish_wire_fetch(DOWN)), _words(reg.publish_wire_fetch(EFFECT))
        assert np.array_equal(down, _expect(reg, DOWN, True)) and np.array_equal(eff, _expect(reg, EFFECT, True))
        out.append((down, eff, rep["effect_num"]))
        reg.close()
    assert out[0][2] == out[1][2] == len(out[1][1]) and out[0][2] > 1000
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_two_deep_lifetime():
    """Scan m's bytes are intact when fetched from while_waiting of call m + 1 (and after it); call m + 2 writes the same buffers."""
    from harness import synth
    w = _world()
    reg = _registrar()
    reg.publish_wire_set(DENSE | EFFECT | BODY, to_host=True)
    scans = []
    for k in range(4):
        s = synth.make_scan(w["hall"], "tiny", w["R"], w["p"] + np.array([0.04, 0.0, 0.0]) * k, noise=0.02, seed=40 + k)
        scans.append(s[np.argsort(s[:, 3], kind="stable")])
    dev = [reg.device_scan(s) for s in scans]
    after, inside = [], []

    def hook():
        if after:
            inside.append([reg.publish_wire_fetch(c) for c in (DENSE, EFFECT, BODY)])

    st = _state()
    for k in range(4):
        reg.scan_register(st, st.copy(), imu_poses=_poses(), leaf=0.2, max_iterations=4, scan_dev=dev[k], scan_sorted=True,
                          next_scan=dev[k + 1] if k + 1 < 4 else None, while_waiting=hook)
        views = [reg.publish_wire_fetch(c, copy=False) for c in (DENSE, EFFECT, BODY)]  # the library's pinned buffers themselves
        after.append(([v.copy() for v in views], views))
    assert len(inside) == 3
    for k in range(3):
        for a, b in zip(inside[k], after[k][0]):
            assert np.array_equal(a, b), k
    for v, c in zip(after[2][1], after[2][0]):
        assert np.array_equal(v, c)  # two deep: call 3 left scan 2's buffers alone ...
    n = min(len(after[1][1][0]), len(after[3][0][0]))
    assert np.array_equal(after[1][1][0][:n], after[3][0][0][:n])  # ... and wrote scan 3's records where scan 1's were
    assert not np.array_equal(after[1][0][0][:n], after[3][0][0][:n])
    reg.close()


@pytest.mark.parametrize("both", [True, False])
def test_publish_now_at_a_callers_state(both):
    import lidar_imu_init_amd as lii
    from harness import synth
    other = lii.State()
    other.rot_end[:] = synth.rot_zyx(0.4, 0.1, -1.0)
    other.pos_end[:] = [7.0, -3.0, 1.5]
    other.offset_T_L_I[:] = [0.1, 0.2, 0.3]
    scan, inten = _take(1000, False), _inten(1000, 21)
    reg = _registrar()
    if both:
        reg.publish_set(ALL | INTENSITY, to_host=True)
    reg.publish_wire_set(ALL, to_host=True)
    assert _code(lambda: reg.publish_now(other)) == STATE  # (no scan yet)
    reg.scan_upload(scan)
    reg.scan_intensity_upload(inten)
    reg.downsample(0.25)
    st = _state()
    reg.iekf_iterate(st, True, False)
    reg.publish_now(other)
    if both:
        got = _check_all(reg, True, "publish_now")
        _cache["now"] = got
    else:
        got = {c: _words(reg.publish_wire_fetch(c)) for c in (DENSE, DOWN, EFFECT, BODY)}
        if "now" in _cache:  # the wire order alone: the same bytes
            for c in got:
                assert np.array_equal(got[c], _cache["now"][c]), c
    assert np.array_equal(got[BODY], _pack(scan, inten, scan[:, 3]))  # feats_undistort as it is
    assert np.array_equal(got[DENSE][:, 8], _bits(inten)) and len(got[EFFECT]) > 0
    reg.close()


def test_rules():
    from lidar_imu_init_amd import api
    reg = _registrar()
    hp, dp, n = C.c_void_p(), C.c_void_p(), C.c_int32(0)
    wfetch = lambda c: reg.L.lii_publish_wire_fetch(reg.h, c, C.byref(hp), C.byref(dp), C.byref(n))
    fetch = lambda c: reg.L.lii_publish_fetch(reg.h, c, C.byref(hp), C.byref(dp), C.byref(n))
    assert wfetch(DENSE) == STATE  # nothing ordered
    for bad in (api.lii_wire_opts(12, 1, 0, 0), api.lii_wire_opts(16, 32, 0, 0), api.lii_wire_opts(16, DENSE | INTENSITY, 0, 0),
                api.lii_wire_opts(16, INTENSITY, 0, 0), api.lii_wire_opts(16, 1, 2, 0), api.lii_wire_opts(16, 1, -1, 0), api.lii_wire_opts(16, 1, 0, 1)):
        assert reg.L.lii_publish_wire_set(reg.h, C.byref(bad)) == INVALID
    assert wfetch(DENSE) == STATE  # (a refused order is no order)
    reg.publish_wire_set(DENSE)
    assert wfetch(DENSE) == STATE  # no registration since the order
    assert wfetch(3) == INVALID and wfetch(16) == INVALID and wfetch(0) == INVALID
    st = _state()

    def register(k=500):
        _register(reg, st, _take(k, True), None, undistort=2, leaf=0.0)

    register()
    assert wfetch(DENSE) == 0 and n.value == 500 and dp.value and not hp.value  # (no to_host: a device pointer only)
    assert _fetch_wire(reg, DENSE, to_host=False).shape == (500, 12)
    assert wfetch(DOWN) == STATE and fetch(DENSE) == STATE  # not ordered
    # placing the other order forgets the clouds of earlier registrations for both ...
    reg.publish_set(DENSE)
    assert wfetch(DENSE) == STATE and fetch(DENSE) == STATE
    register()
    assert wfetch(DENSE) == 0 and fetch(DENSE) == 0
    # ... and so does placing (changing) this one
    reg.publish_wire_set(DENSE | DOWN)
    assert wfetch(DENSE) == STATE and fetch(DENSE) == STATE
    register()
    assert wfetch(DOWN) == 0 and n.value == 500 and fetch(DENSE) == 0
    # off: the other order goes on; on again: the buffers are still there
    reg.publish_wire_set(0)
    assert wfetch(DENSE) == STATE
    register()
    assert wfetch(DENSE) == STATE and fetch(DENSE) == 0
    reg.publish_wire_set(DOWN)
    register(300)
    assert wfetch(DOWN) == 0 and n.value == 300 and wfetch(DENSE) == STATE
    # not from inside a registration
    codes = []
    reg.scan_upload(_take(300, True))
    reg.scan_register(st, st.copy(), cv=True, leaf=0.0, max_iterations=2, scan_sorted=True,
                      while_waiting=lambda: codes.append((_code(lambda: reg.publish_wire_set(DENSE)), _code(lambda: reg.publish_saved_pcd()), wfetch(DOWN))))
    assert codes == [(STATE, STATE, 0)]
    assert reg.L.lii_publish_saved_pcd(reg.h, None, 0, C.byref(n), 0) == STATE  # no save buffer
    reg.close()
    # a communicator attached: single rank only for now; without it the order is taken
    reg = _registrar()
    reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")
    assert _code(lambda: reg.publish_wire_set(DENSE)) == STATE
    reg.comm_destroy()
    assert _code(lambda: reg.publish_wire_set(DENSE)) == 0
    reg.close()
    reg = _registrar(env="host_solve")
    assert _code(lambda: reg.publish_wire_set(DENSE)) == STATE
    reg.close()


def _pcd(reg, clear=0):
    """(status, rows as (n, 8) uint32) of lii_publish_saved_pcd"""
    n = C.c_int32(0)
    reg.L.lii_publish_saved_pcd(reg.h, None, 0, C.byref(n), 0)
    rows = np.zeros((max(n.value, 1), 8), np.uint32)
    rc = reg.L.lii_publish_saved_pcd(reg.h, rows.ctypes.data_as(C.c_void_p), rows.nbytes, C.byref(n), clear)
    return rc, rows[:n.value]


def _pcd_pack(cloud4, inten):
    """x y z | normal 0 0 0 | intensity | curvature 0"""
    rows = np.zeros((len(cloud4), 8), np.uint32)
    rows[:, 0:3] = _bits(cloud4[:, :3]).reshape(-1, 3)
    rows[:, 6] = _bits(inten)
    return rows


def test_pcd_rows():
    reg = _registrar()
    reg.publish_set(DENSE | INTENSITY, to_host=True, save_capacity=257 + 1000 + 499)  # the third scan (500) does not fit
    st = _state(2)
    for k, m in enumerate((257, 1000)):
        _register(reg, st, _take(m, True), _inten(m, 30 + k), undistort=2, leaf=0.3)
    rc, rows = _pcd(reg)
    cloud, it = reg.publish_saved(), reg.publish_saved_intensity()
    assert rc == 0 and len(cloud) == 1257 and it.all()
    assert np.array_equal(rows, _pcd_pack(cloud, it))
    assert np.array_equal(reg.publish_saved_pcd().view(np.uint32).reshape(-1, 8), rows)
    # capacity in bytes: one byte short is refused, nothing is cleared
    cnt, short = C.c_int32(0), np.zeros(32 * 1257 - 1, np.uint8)
    assert reg.L.lii_publish_saved_pcd(reg.h, short.ctypes.data_as(C.c_void_p), short.nbytes, C.byref(cnt), 1) == CAPACITY and cnt.value == 1257
    assert not short.any()
    _register(reg, st, _take(500, True), _inten(500, 32), undistort=2, leaf=0.3)
    rc, rows2 = _pcd(reg)
    cnt4 = C.c_int32(0)
    assert rc == CAPACITY == reg.L.lii_publish_saved(reg.h, None, 0, C.byref(cnt4), 0) and cnt4.value == 1257  # sticky, as lii_publish_saved reports it
    assert np.array_equal(rows2, rows)  # what the buffer held is intact
    rc, rows3 = _pcd(reg, clear=1)
    assert rc == CAPACITY and np.array_equal(rows3, rows)
    rc, rows4 = _pcd(reg)
    assert rc == 0 and len(rows4) == 0 and len(reg.publish_saved()) == 0 and len(reg.publish_saved_intensity()) == 0  # `clear` emptied both
    reg.close()


def test_pcd_rows_across_the_staging_chunk_and_without_intensities():
    """65 537 points: five scans of 16 384, the last cut to one point - row 65 536 comes through the second chunk of the staging area."""
    full = _take(16_384, True)
    reg = _registrar()
    reg.publish_set(DENSE | INTENSITY, save_capacity=65_537)
    st = _state(2)
    for k in range(5):
        s = full.copy() if k < 4 else full[:1].copy()
        s[:, :3] *= np.float32(1.0 + 0.002 * k)
        _register(reg, st, s, _inten(len(s), 50 + k), undistort=2, leaf=0.3)
    rc, rows = _pcd(reg)
    cloud, it = reg.publish_saved(), reg.publish_saved_intensity()
    exp = _pcd_pack(cloud, it)
    assert rc == 0 and rows.shape == (65_537, 8) and it.all()
    assert np.array_equal(rows[65_535], exp[65_535]) and np.array_equal(rows[65_536], exp[65_536])
    assert rows[65_536, 0:3].any() and rows[65_536, 6] != 0
    assert np.array_equal(rows, exp)
    reg.close()
    # a save buffer built without LII_PUB_INTENSITY: intensity 0, whatever the scan carries
    reg = _registrar()
    reg.publish_set(DENSE, save_capacity=3000)
    _register(reg, st, _take(1000, True), _inten(1000, 60), undistort=2, leaf=0.3)
    rc, rows = _pcd(reg)
    assert rc == 0 and np.array_equal(rows, _pcd_pack(reg.publish_saved(), np.zeros(1000, np.float32))) and rows[:, 0].any()
    reg.close()
