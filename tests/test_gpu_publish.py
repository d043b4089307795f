"""The registered clouds of a scan (lii_publish_set / _now / _fetch / _saved; lii_publish.hip: k_publish_world) - what laserMapping's
loop hands out behind the update, src/laserMapping.cpp:1152-1156: publish_frame_world (:561-614), publish_frame_body (:616-623),
publish_effect_world (:625-636), the pcl_wait_save append (:594-613).

Reference: the oracle's restatement of pointBodyToWorld (oracle/orc_iekf.hpp:68-74 = src/laserMapping.cpp:209-220; held against the
written-out double formula in tests/test_publish_cabi.py) applied to what lii_scan_download returns, at the state the call RETURNED.
Every comparison is bit for bit (uint32 views): both sides do the same double arithmetic without contraction and round to float once.
Worlds: harness/synth.py halls with maps of a few thousand points."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, CAPACITY, STATE = -1, -4, -5
DENSE, DOWN, EFFECT, BODY = 1, 2, 4, 8
MAX_SCAN = 20_000
_cache = {}


def _world():
    """hall, map points (a few thousand), true pose, a 16 384-ray scan from it, a start state a little off."""
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
        st.offset_R_L_I[:] = synth.rot_zyx(0.01, -0.02, 0.015)  # (a non-trivial extrinsic: both halves of pointBodyToWorld count)
        st.offset_T_L_I[:] = [0.04, -0.02, 0.05]
        st.gravity[:] = [0, 0, -9.81]
        _cache["w"] = dict(hall=hall, map=map_pts, R=R, p=p, scan=scan, st=st)
        print(f"world: map {len(map_pts)} points, scan {len(scan)} points")
    return _cache["w"]


def _registrar(**kw):
    import lidar_imu_init_amd as lii
    w = _world()
    reg = lii.Registrar(**{**dict(max_scan_points=MAX_SCAN, max_map_points=max(4 * len(w["map"]), 50_000), filter_size_map=0.15), **kw})
    reg.map_build(w["map"])
    return reg


def _to_world(state, pts4):
    """pointBodyToWorld by the oracle at `state` (one pass of its update on a tiny tree fills `world`), t_ms carried through."""
    from oracle import oracle as O
    if "tree" not in _cache:
        _cache["tree"] = O.Tree("oracle")
        _cache["tree"].build(np.random.default_rng(1).normal(size=(32, 3)).astype(np.float32))
    pts4 = np.ascontiguousarray(pts4, np.float32)
    if len(pts4) == 0:
        return np.zeros((0, 4), np.float32)
    out = pts4.copy()
    out[:, :3] = _cache["tree"].iekf_update(pts4, state.pod, state.pod, max_iterations=1)["world"]
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rows_sorted(a):
    b = _bits(a).reshape(-1, 4)
    return b[np.lexsort(b.T[::-1])]


def _poses():
    """A short IMUpose table (offset_time, acc, gyr, vel, pos, rot) with a little motion over the 100 ms sweep."""
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
    """n points of the scan, spread over the sweep: in ascending time order, or in the scan's own (ring-major) order."""
    s = _world()["scan"]
    idx = np.linspace(0, len(s) - 1, n).astype(int) if n > 1 else np.array([len(s) // 2])
    s = s[idx]
    return s[np.argsort(s[:, 3], kind="stable")] if sorted_ else s


def _code(fn):
    import lidar_imu_init_amd as lii
    try:
        fn()
    except lii.LIIError as e:
        return e.code
    return 0


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
@pytest.mark.parametrize("undistort", [1, 2])
@pytest.mark.parametrize("sorted_", [True, False])
def test_dense_and_body_clouds(n, undistort, sorted_):
    reg = _registrar()
    reg.publish_set(DENSE | BODY, to_host=True)
    scan = _take(n, sorted_)
    assert sorted_ or n < 3 or not np.all(np.diff(scan[:, 3]) >= 0)
    st = _world()["st"].copy()
    if undistort == 2:
        st.bias_g[:] = [0.02, -0.01, 0.05]
        st.vel_end[:] = [0.3, -0.2, 0.05]
    reg.scan_upload(scan)
    kw = dict(imu_poses=_poses()) if undistort == 1 else dict(cv=True)
    rep = reg.scan_register(st, st.copy(), leaf=0.2, max_iterations=4, scan_sorted=sorted_, **kw)
    dense = reg.publish_fetch(DENSE)
    body = reg.publish_fetch(BODY)
    deskewed = reg.scan_download(0)
    print(f"n {n} undistort {undistort} sorted {sorted_}: iterations {rep['iterations']} effect {rep['effect_num']}; dense {dense.shape}")
    assert dense.shape == (n, 4) and body.shape == (n, 4)
    assert np.array_equal(_bits(body), _bits(deskewed))
    ref = _to_world(st, deskewed)
    assert np.array_equal(_bits(dense[:, 3]), _bits(scan[:, 3]))  # t_ms of the input, in the input's order
    assert np.array_equal(_bits(dense[:, 3]), _bits(deskewed[:, 3]))
    assert np.array_equal(_bits(dense), _bits(ref)), int((_bits(dense) != _bits(ref)).sum())
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


@pytest.mark.parametrize("target", [200, 257, 3000])
def test_down_sampled_and_effect_clouds(target):
    """Down-sampled sizes on both sides of one workgroup and over several; no de-skew, so that the voxel count is the oracle's."""
    leaf = 0.25
    scan = _prefix_for_voxels(target, leaf)
    runs = []
    for _ in range(2):
        reg = _registrar()
        reg.publish_set(DOWN | EFFECT, to_host=False)
        st = _world()["st"].copy()
        reg.scan_upload(scan)
        rep = reg.scan_register(st, st.copy(), leaf=leaf, max_iterations=4, scan_sorted=True)
        down = reg.publish_fetch(DOWN)
        eff = reg.publish_fetch(EFFECT)
        body = reg.scan_download(1)
        _, _, sel = reg.neighbors(len(body))
        runs.append((down, eff, st.pod.copy()))
        reg.close()
    print(f"target {target}: scan {len(scan)} -> down-sampled {len(down)}, effect {len(eff)} (report {rep['effect_num']})")
    assert len(down) == len(body) and abs(len(down) - target) <= 2
    ref = _to_world(st, body)
    assert np.array_equal(_rows_sorted(down), _rows_sorted(ref))
    assert len(eff) == rep["effect_num"] == int(sel.sum())
    assert np.array_equal(_rows_sorted(eff), _rows_sorted(ref[sel != 0]))
    # ascending index of the device's order: the effect cloud is a subsequence of the down-sampled cloud
    pos = {r.tobytes(): i for i, r in enumerate(_bits(down))}
    at = [pos[r.tobytes()] for r in _bits(eff)]
    assert at == sorted(at)
    # the same bits in the same order on a second run
    assert np.array_equal(runs[0][2], runs[1][2])
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))


def test_effect_cloud_nothing_and_almost_everything_selected():
    from harness import synth
    w = _world()
    reg = _registrar()
    reg.publish_set(DOWN | EFFECT, to_host=True)
    # far from the map: no neighbour within reach, nothing is selected
    far = w["st"].copy()
    far.pos_end[:] += [500.0, 0, 0]
    reg.scan_upload(_take(3000, True))
    rep = reg.scan_register(far, far.copy(), leaf=0.0, max_iterations=3, scan_sorted=True)
    eff = reg.publish_fetch(EFFECT)
    assert rep["effect_num"] == 0 and eff.shape == (0, 4) and len(reg.publish_fetch(DOWN)) == 3000
    # a noise-free scan from the true pose against a dense noise-free map: (almost) every point is selected
    reg2 = _registrar(max_map_points=400_000)
    reg2.map_build(w["hall"].surface_points(0.1, noise=0.0, seed=3))
    reg2.publish_set(EFFECT, to_host=True)
    import lidar_imu_init_amd as lii
    st = lii.State()
    st.rot_end[:] = w["R"]
    st.pos_end[:] = w["p"]
    scan = synth.make_scan(w["hall"], "tiny", w["R"], w["p"], noise=0.0, seed=5)
    reg2.scan_upload(scan)
    rep = reg2.scan_register(st, st.copy(), leaf=0.0, max_iterations=3)
    eff = reg2.publish_fetch(EFFECT)
    print(f"almost everything: {len(eff)} of {len(scan)} selected")
    # (a point within a map spacing or two of an edge has neighbours on two faces and fails the plane test: a few per cent of a sweep,
    # 20 % allowed)
    assert len(eff) == rep["effect_num"] and len(eff) > 0.8 * len(scan)
    _, _, sel = reg2.neighbors(len(scan))
    assert np.array_equal(_bits(eff), _bits(_to_world(st, scan)[sel != 0]))  # (no filter: the device's order is the scan's)
    reg.close()
    reg2.close()


def _imu_rows(t_beg):
    t = t_beg + np.arange(0, 11) * 0.01
    rows = np.zeros((len(t), 7))
    rows[:, 0] = t
    rows[:, 1:4] = [0.01, -0.02, 0.03]
    rows[:, 4:7] = [0.05, -0.03, 9.81]
    return rows


def _six_scans(form, publish, profile=False, cancel_order=False):
    """Six consecutive scans with the map update inside the call; returns everything a caller can see of them."""
    from harness import synth
    w = _world()
    reg = _registrar()
    if publish:
        reg.publish_set(DENSE | DOWN | EFFECT | BODY, to_host=True, save_capacity=3 * MAX_SCAN)
    if cancel_order:
        reg.publish_set(DENSE | DOWN | EFFECT | BODY, to_host=True, save_capacity=1000)
        reg.publish_set(0)
    if profile:
        reg.set_profiling(1)
        reg.set_profiling(3)
    if form == "imu":
        reg.set_imu_noise(cov_gyr=0.1, cov_acc=0.1, mean_acc_norm=9.81)
        reg.imu_carry = dict(last_imu=np.r_[99.99, 0.01, -0.02, 0.03, 0.05, -0.03, 9.81], last_lidar_end_time=99.995)
    st = w["st"].copy()
    st.bias_g[:] = 0 if form != "cv" else [0.01, -0.02, 0.03]
    out = []
    for k in range(6):
        Rk = w["R"] @ synth.rot_zyx(0.0, 0.0, 0.01 * k)
        pk = w["p"] + np.array([0.05, 0.02, 0.0]) * k
        scan = synth.make_scan(w["hall"], "tiny", Rk, pk, noise=0.02, seed=20 + k)
        scan = scan[np.argsort(scan[:, 3], kind="stable")]
        dev = reg.device_scan(scan)
        if form == "poses":
            rep = reg.scan_register(st, st.copy(), imu_poses=_poses(), leaf=0.2, max_iterations=4, scan_dev=dev, scan_sorted=True, map_update=True)
        elif form == "cv":
            _, _, rep = reg.register_cv(0.1, 1.0, 1.0, st, leaf=0.2, max_iterations=4, scan_dev=dev, scan_sorted=True, map_update=True)
        else:
            _, _, rep = reg.register_imu(_imu_rows(100.0 + 0.1 * k), 100.0 + 0.1 * k, st, leaf=0.2, max_iterations=4, imu_en=True, scan_dev=dev,
                                         scan_sorted=True, map_update=True)
        out.append((st.pod.tobytes(), rep["iterations"], rep["searches"], rep["effect_num"], rep["normal_eq"].tobytes(), reg.last_unfinished_queries()))
    m = reg.map_download()
    prof = reg.kernel_profile() if profile else None
    reg.close()
    return out, _rows_sorted(np.c_[m[:, :3], np.zeros(len(m))]), prof


@pytest.mark.parametrize("form", ["poses", "cv", "imu"])
def test_publishing_changes_nothing_else(form):
    a, map_a, _ = _six_scans(form, False)
    b, map_b, _ = _six_scans(form, True)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x[1:4] == y[1:4] and x[5] == y[5], (form, k, x[1:4], y[1:4])
        assert x[0] == y[0] and x[4] == y[4], (form, k)
    assert np.array_equal(map_a, map_b)


def test_an_order_that_is_off_adds_no_launch():
    """lii_set_profiling(h, 3): a handle whose order was placed and taken back launches what a handle without one launches;
    with the order on, one launch per scan is attributed to the kind of its own."""
    _, _, never = _six_scans("poses", False, profile=True)
    _, _, off = _six_scans("poses", False, profile=True, cancel_order=True)
    _, _, on = _six_scans("poses", True, profile=True)
    print("launches, never ordered:", {k: v[1] for k, v in never[0].items()})
    assert {k: v[1] for k, v in never[0].items()} == {k: v[1] for k, v in off[0].items()}
    assert never[0]["publish"][1] == 0 and on[0]["publish"][1] == on[1] == 6
    assert {k: v[1] for k, v in on[0].items() if k != "publish"} == {k: v[1] for k, v in never[0].items() if k != "publish"}


def test_a_parked_loop_publishes_the_final_state():
    """A launch plan that is wrong on purpose (LII_TEST=plan_force=1: only the first pass has its search launch - the re-match parks
    the loop, tests/test_gpu_launch_plan.py): the launch behind the planned passes finds a parked loop and does nothing, the one
    behind the continued loop publishes - at the state the call returns."""
    old = os.environ.get("LII_TEST")
    os.environ["LII_TEST"] = "plan_force=1"
    try:
        reg = _registrar()
    finally:
        os.environ.pop("LII_TEST", None)
        if old is not None:
            os.environ["LII_TEST"] = old
    reg.publish_set(DENSE | DOWN | EFFECT, to_host=True, save_capacity=MAX_SCAN)
    for k in range(2):
        st = _world()["st"].copy()
        scan = _take(4099, True)
        reg.scan_upload(scan)
        rep = reg.scan_register(st, st.copy(), imu_poses=_poses(), leaf=0.2, max_iterations=5, scan_sorted=True)
        assert rep["searches"] >= 2  # (the re-match ran: the plan did not hold it)
        dense, down, eff = reg.publish_fetch(DENSE), reg.publish_fetch(DOWN), reg.publish_fetch(EFFECT)
        assert np.array_equal(_bits(dense), _bits(_to_world(st, reg.scan_download(0))))
        assert np.array_equal(_rows_sorted(down), _rows_sorted(_to_world(st, reg.scan_download(1))))
        assert len(eff) == rep["effect_num"]
    saved = reg.publish_saved()
    assert len(saved) == 2 * 4099 and np.array_equal(_bits(saved[4099:]), _bits(dense))  # (appended once per scan, by the launch that published)
    reg.close()


def test_fetch_of_scan_m_inside_call_m_plus_1():
    """lii_publish_fetch from lii_scan_job::while_waiting of the next call: scan m's clouds, intact, while scan m + 1 is registered."""
    from harness import synth
    w = _world()
    reg = _registrar()
    reg.publish_set(DENSE | EFFECT, to_host=True)
    scans = []
    for k in range(4):
        s = synth.make_scan(w["hall"], "tiny", w["R"], w["p"] + np.array([0.04, 0.0, 0.0]) * k, noise=0.02, seed=40 + k)
        scans.append(s[np.argsort(s[:, 3], kind="stable")])
    dev = [reg.device_scan(s) for s in scans]
    after, inside = [], []

    def hook():
        if after:
            inside.append((reg.publish_fetch(DENSE), reg.publish_fetch(EFFECT)))

    st = w["st"].copy()
    for k in range(4):
        reg.scan_register(st, st.copy(), imu_poses=_poses(), leaf=0.2, max_iterations=4, scan_dev=dev[k], scan_sorted=True,
                          next_scan=dev[k + 1] if k + 1 < 4 else None, while_waiting=hook)
        view = reg.publish_fetch(DENSE, copy=False)  # the library's pinned buffer itself: must still hold scan k after call k + 1
        after.append((view.copy(), reg.publish_fetch(EFFECT), view, st.copy()))
    assert len(inside) == 3
    for k in range(3):
        assert np.array_equal(_bits(inside[k][0]), _bits(after[k][0])) and np.array_equal(_bits(inside[k][1]), _bits(after[k][1]))
    assert np.array_equal(_bits(after[2][2]), _bits(after[2][0]))  # (two deep: scan 2's buffer is untouched by call 3)
    reg.close()


def test_fetching_does_not_end_a_pre_armed_launch():
    """As tests/test_gpu_prearm.py tells the two forms apart (LII_DIAG's count at lii_destroy), in a child process: every call announces
    its successor and fetches the clouds right behind the call and inside the next call's hook - the pre-armed prologues are still used."""
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
import lidar_imu_init_amd as lii
from harness import synth
hall = synth.Hall(size=(20.0, 16.0, 6.0), n_boxes=6, seed=3)
R = synth.rot_zyx(0.02, -0.01, 0.3); p = np.array([0.5, -0.4, 0.1])
reg = lii.Registrar(max_scan_points=4096, max_map_points=100000, filter_size_map=0.15)
reg.map_build(hall.surface_points(0.3, noise=0.01, seed=3)); reg.map_commit()
reg.publish_set(1 | 2 | 4 | 8, to_host=True)
scans = []
for k in range(6):
    s = synth.make_scan(hall, "tiny", R, p + np.array([0.03, 0, 0]) * k, noise=0.02, seed=60 + k)
    scans.append(s[np.argsort(s[:, 3], kind="stable")])
dev = [reg.device_scan(s) for s in scans]
P = np.zeros((3, 22)); P[:, 0] = [0, 0.05, 0.1]; P[:, 13] = P[:, 17] = P[:, 21] = 1.0
st = lii.State(); st.rot_end[:] = R; st.pos_end[:] = p
got = []
for k in range(6):
    reg.scan_register(st, st.copy(), imu_poses=P, leaf=0.2, max_iterations=4, imu_en=False, scan_dev=dev[k], scan_sorted=True,
                      next_scan=dev[k + 1] if k + 1 < 6 else None, while_waiting=lambda: got.append(len(reg.publish_fetch(1))) if k else None)
    for c in (1, 2, 4, 8):
        reg.publish_fetch(c)
reg.close()
print("OK", got)
''' % ROOT
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LII_DIAG="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
    import re
    used = int(re.search(r"pre-armed prologues: (\d+) used", r.stderr).group(1))
    assert used >= 4, r.stderr[-600:]  # (five announcements; the sibling test allows one of nine to end for the voxel filter's change of form)


def test_upload_pipeline_with_device_only_clouds():
    """The documented pipeline - lii_scan_upload_next, lii_scan_register with the map update in the job, lii_scan_advance - with
    DENSE | BODY ordered, to_host = 0 and a save buffer: the launch and the body copy of scan k read the scan buffer behind the stopping
    pass, and the transfer of scan k + 2 into that very buffer must come behind them.  Every scan's clouds are fetched AFTER the next
    transfer has been started and compared bit for bit with a run that uploads every scan by itself."""
    n, k_scans = 16_000, 6
    full = _take(len(_world()["scan"]), True)[:n]
    scans = []
    for k in range(k_scans):  # as many points every time, all different: a row of another scan cannot pass for this one's
        s = full.copy()
        s[:, :3] *= np.float32(1.0 + 0.002 * k)
        scans.append(np.ascontiguousarray(s))

    def register(reg, st):
        return reg.scan_register(st, st.copy(), imu_poses=_poses(), leaf=0.3, max_iterations=3, scan_sorted=True, map_update=True)

    ref = []
    reg = _registrar()
    reg.publish_set(DENSE | BODY, to_host=False, save_capacity=k_scans * n)
    st = _world()["st"].copy()
    for k in range(k_scans):
        reg.scan_upload(scans[k])
        register(reg, st)
        ref.append((reg.publish_fetch(DENSE), reg.publish_fetch(BODY), st.pod.copy()))
    ref_saved = reg.publish_saved()
    reg.close()
    reg = _registrar()
    reg.publish_set(DENSE | BODY, to_host=False, save_capacity=k_scans * n)
    st = _world()["st"].copy()

    def check(k):
        dense, body = reg.publish_fetch(DENSE), reg.publish_fetch(BODY)
        assert np.array_equal(_bits(body), _bits(ref[k][1])), (k, int((_bits(body) != _bits(ref[k][1])).any(axis=1).sum()))
        assert np.array_equal(_bits(dense), _bits(ref[k][0])), (k, int((_bits(dense) != _bits(ref[k][0])).any(axis=1).sum()))

    reg.scan_upload_next(scans[0])
    reg.scan_advance()
    for k in range(k_scans):
        if k + 1 < k_scans:
            reg.scan_upload_next(scans[k + 1])  # into the buffer scan k - 1 was registered in
        if k >= 1:
            check(k - 1)  # (scan k - 1's clouds, fetched with that transfer started)
        register(reg, st)
        assert np.array_equal(st.pod, ref[k][2]), k
        if k + 1 < k_scans:
            reg.scan_advance()
    check(k_scans - 1)
    assert np.array_equal(_bits(reg.publish_saved()), _bits(ref_saved))
    reg.close()


def test_effect_cloud_with_late_count_words():
    """LII_TEST=emit_late: every seventh workgroup of the down-sampled cloud publishes its count word late and the workgroups above it
    count its block themselves (prefix_below's path for a launch whose workgroups are not all resident): the same clouds, bit for bit."""
    scan = _take(8000, True)  # leaf 0: 8 000 down-sampled points, 32 workgroups
    out = []
    for env in (None, "emit_late"):
        old = os.environ.get("LII_TEST")
        os.environ.pop("LII_TEST", None)
        if env:
            os.environ["LII_TEST"] = env
        try:
            reg = _registrar()
        finally:
            os.environ.pop("LII_TEST", None)
            if old is not None:
                os.environ["LII_TEST"] = old
        reg.publish_set(DOWN | EFFECT, to_host=True)
        st = _world()["st"].copy()
        reg.scan_upload(scan)
        rep = reg.scan_register(st, st.copy(), leaf=0.0, max_iterations=4, scan_sorted=True)
        out.append((reg.publish_fetch(DOWN), reg.publish_fetch(EFFECT), rep["effect_num"], st.pod.copy()))
        reg.close()
    assert out[0][2] == out[1][2] == len(out[1][1]) and out[0][2] > 1000
    assert np.array_equal(out[0][3], out[1][3])
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(_bits(out[0][1]), _bits(out[1][1]))


def test_save_buffer():
    n = 2000
    reg = _registrar()
    reg.publish_set(DENSE, to_host=True, save_capacity=4 * n - 1)
    clouds = []
    st = _world()["st"].copy()

    def one(k):
        s = _take(n, True).copy()
        s[:, 0] += 0.01 * k
        reg.scan_upload(s)
        reg.scan_register(st, st.copy(), cv=True, leaf=0.3, max_iterations=3, scan_sorted=True)
        return reg.publish_fetch(DENSE)

    for k in range(3):
        clouds.append(one(k))
    saved = reg.publish_saved()
    assert np.array_equal(_bits(saved), _bits(np.concatenate(clouds)))
    # too small a capacity: LII_ERR_CAPACITY, nothing is cleared
    small, cnt = np.zeros((10, 4), np.float32), C.c_int32(0)
    assert reg.L.lii_publish_saved(reg.h, small.ctypes.data, 10, C.byref(cnt), 1) == CAPACITY and cnt.value == 3 * n
    assert len(reg.publish_saved()) == 3 * n
    # a fourth scan does not fit: reported, the three are intact, the handle goes on working
    fourth = one(3)
    assert fourth.shape == (n, 4)
    out, cnt = np.zeros((4 * n, 4), np.float32), C.c_int32(0)
    assert reg.L.lii_publish_saved(reg.h, out.ctypes.data, 4 * n, C.byref(cnt), 0) == CAPACITY
    assert cnt.value == 3 * n and np.array_equal(_bits(out[:3 * n]), _bits(np.concatenate(clouds)))
    assert reg.L.lii_publish_saved(reg.h, out.ctypes.data, 4 * n, C.byref(cnt), 1) == CAPACITY  # (sticky until cleared)
    assert len(reg.publish_saved()) == 0  # `clear` emptied the buffer and took the flag down
    fifth = one(4)
    assert np.array_equal(_bits(reg.publish_saved(clear=True)), _bits(fifth)) and len(reg.publish_saved()) == 0
    reg.close()


def test_publish_now_at_a_callers_state():
    import lidar_imu_init_amd as lii
    from harness import synth
    reg = _registrar()
    reg.publish_set(DENSE | DOWN | EFFECT | BODY)
    scan = _take(1000, False)
    reg.scan_upload(scan)
    reg.downsample(0.25)
    st = _world()["st"].copy()
    reg.iekf_iterate(st, True, False)
    other = lii.State()
    other.rot_end[:] = synth.rot_zyx(0.4, 0.1, -1.0)
    other.pos_end[:] = [7.0, -3.0, 1.5]
    other.offset_T_L_I[:] = [0.1, 0.2, 0.3]
    reg.publish_now(other)
    body = reg.scan_download(1)
    _, _, sel = reg.neighbors(len(body))
    assert np.array_equal(_bits(reg.publish_fetch(DENSE)), _bits(_to_world(other, scan)))
    assert np.array_equal(_bits(reg.publish_fetch(BODY)), _bits(scan))
    assert np.array_equal(_rows_sorted(reg.publish_fetch(DOWN)), _rows_sorted(_to_world(other, body)))
    assert np.array_equal(_rows_sorted(reg.publish_fetch(EFFECT)), _rows_sorted(_to_world(other, body)[sel != 0])) and sel.sum() > 0
    reg.close()


def test_refusals():
    from lidar_imu_init_amd import api
    reg = _registrar()
    hp, dp, n = C.c_void_p(), C.c_void_p(), C.c_int32(0)
    fetch = lambda c: reg.L.lii_publish_fetch(reg.h, c, C.byref(hp), C.byref(dp), C.byref(n))
    assert fetch(DENSE) == STATE  # nothing ordered
    assert _code(lambda: reg.publish_now(_world()["st"])) == STATE
    assert reg.L.lii_publish_saved(reg.h, None, 0, C.byref(n), 0) == STATE  # no save buffer
    for bad in (api.lii_publish_opts(12, 1, 0, 0), api.lii_publish_opts(16, 16, 0, 0), api.lii_publish_opts(16, 1, 2, 0), api.lii_publish_opts(16, 1, 0, -1)):
        assert reg.L.lii_publish_set(reg.h, C.byref(bad)) == INVALID
    reg.publish_set(DENSE)
    assert fetch(DENSE) == STATE  # no registration since the order
    assert fetch(3) == INVALID and fetch(16) == INVALID and fetch(0) == INVALID
    st = _world()["st"].copy()
    reg.scan_upload(_take(500, True))
    reg.scan_register(st, st.copy(), cv=True, leaf=0.0, max_iterations=2, scan_sorted=True)
    assert fetch(DENSE) == 0 and n.value == 500 and dp.value and not hp.value  # (no to_host: a device pointer only)
    assert fetch(DOWN) == STATE  # not ordered
    reg.publish_set(0)  # off ...
    assert fetch(DENSE) == STATE
    reg.scan_upload(_take(500, True))
    reg.scan_register(st, st.copy(), cv=True, leaf=0.0, max_iterations=2, scan_sorted=True)
    assert fetch(DENSE) == STATE
    reg.publish_set(DENSE | DOWN)  # ... and on again: the buffers of the first order are still there
    reg.scan_upload(_take(500, True))
    reg.scan_register(st, st.copy(), cv=True, leaf=0.0, max_iterations=2, scan_sorted=True)
    assert fetch(DENSE) == 0 and fetch(DOWN) == 0 and n.value == 500
    reg.close()
    # a communicator attached: single rank only for now; without it the order is taken again
    reg = _registrar()
    reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")
    assert _code(lambda: reg.publish_set(DENSE)) == STATE
    assert _code(lambda: reg.publish_set(0, save_capacity=100)) == STATE
    reg.comm_destroy()
    assert _code(lambda: reg.publish_set(DENSE)) == 0
    reg.close()
    # LII_TEST=host_solve: single rank, device-driven loop only
    old = os.environ.get("LII_TEST")
    os.environ["LII_TEST"] = "host_solve"
    try:
        reg = _registrar()
    finally:
        os.environ.pop("LII_TEST", None)
        if old is not None:
            os.environ["LII_TEST"] = old
    assert _code(lambda: reg.publish_set(DENSE)) == STATE
    reg.close()


def test_lifecycle_returns_the_device_memory():
    """Create, order everything, register, destroy - three times in one process; the device memory in use (read as
    tests/test_gpu_handle_lifecycle.py reads it) returns to its value after the first cycle, within one scan buffer."""
    import torch

    def cycle():
        reg = _registrar()
        reg.publish_set(DENSE | DOWN | EFFECT | BODY, to_host=True, save_capacity=2 * MAX_SCAN)
        st = _world()["st"].copy()
        reg.scan_upload(_take(4099, True))
        reg.scan_register(st, st.copy(), cv=True, leaf=0.2, max_iterations=3, scan_sorted=True)
        assert len(reg.publish_fetch(DENSE)) == 4099
        reg.close()
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free

    cycle()  # warm-up: the runtime's own pools
    used = [cycle() for _ in range(3)]
    print("device memory in use after each close:", used)
    assert used[2] - used[0] <= 16 * MAX_SCAN, used  # (the order alone holds 10 buffers of that size: a leak of one per cycle shows)
