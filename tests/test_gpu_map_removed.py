"""The history of what box deletes remove (lii_map_removed_*: points_cache_collect / acquire_removed_points, src/laserMapping.cpp:249-254,
include/ikd-Tree/ikd_Tree.cpp:522-534) on the device.  Every comparison is exact: rows sorted, multisets of float bits
(map_removed_cases.same_multiset); the expectation is numpy's min <= p < max, which test_map_removed_abi.py holds to the reference tree.

  1. lii_map_delete_boxes with the order on, every shared case;
  2. the moving local map, in a job (lii_scan_register, _cv, _imu with map_update = 0) and stand-alone, over local_map_cases' traverse;
  3. overflow;  4. what must not collect;  5. acquire, clear, view, re-setting;  6. off is off (results, map, launch counts per kind);
  7. the refusals;  8. the replay host's switch and its global map."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_removed_cases as MC
from local_map_cases import CUBE_LEN, DET_RANGE, Stream

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, STATE = -1, -4, -5
LEAF, MAX_IT = 0.25, 5
BIG = 50_000
_cache = {}


def _registrar(**kw):
    import lidar_imu_init_amd as lii
    return lii.Registrar(**{**dict(max_scan_points=8_000, max_map_points=60_000, filter_size_map=MC.FILTER_SIZE_MAP), **kw})


def _stream():
    if "s" not in _cache:
        _cache["s"] = Stream()
    return _cache["s"]


def _raw_acquire(reg, capacity, clear):
    """(status, points delivered) of lii_map_removed_acquire with a buffer of `capacity` points"""
    out = np.full((max(capacity, 1), 3), np.nan, np.float32)
    n = C.c_int32(-1)
    rc = reg.L.lii_map_removed_acquire(reg.h, out.ctypes.data_as(C.c_void_p), capacity, C.byref(n), int(clear))
    return rc, out[:max(n.value, 0)] if rc in (0, CAPACITY) and n.value <= capacity else out[:0], n.value


# --------------------------------------------------------------------------------------------------------------------------- 5
def test_acquire_view_and_resetting(small_world):
    """(First in the file: torch, which reads the view, brings a HIP runtime of its own and wants to be in the process before the
    library's - the order the whole suite has anyway - or the second of the two runtimes sees no device.)"""
    import torch
    pts, cases = MC.world(small_world)
    boxes, dead = cases["overlap3"]
    reg = _registrar()
    reg.map_build(pts)
    reg.map_removed_set(BIG)
    assert reg.map_removed_acquire().shape == (0, 3) and reg.map_removed_view() == (None, 0)
    reg.map_delete_boxes(boxes)
    a, b = reg.map_removed_acquire(), reg.map_removed_acquire()
    assert len(a) == int(dead.sum()) and np.array_equal(a.view(np.uint32), b.view(np.uint32))  # clear = 0 twice: the same points
    assert MC.same_multiset(a, pts[dead])
    v, n = reg.map_removed_view()
    t = torch.as_tensor(v, device="cuda").cpu().numpy()
    assert t.shape == (len(a), 4) and MC.same_multiset(t[:, :3], a)
    n_ = C.c_int32(0)
    assert reg.L.lii_map_removed_acquire(reg.h, None, 0, C.byref(n_), 1) == 0 and n_.value == len(a)  # xyz_out == NULL: *n only
    assert reg.map_removed_get()["held"] == len(a)
    rc, _, n_small = _raw_acquire(reg, len(a) - 1, clear=True)
    assert rc == CAPACITY and n_small == len(a) and reg.map_removed_get()["held"] == len(a)  # capacity < *n: nothing cleared
    reg.map_removed_set(BIG)  # the same capacity: the contents stay
    assert MC.same_multiset(reg.map_removed_acquire(), a)
    reg.map_removed_set(0)  # off: readable, and a delete is not collected
    assert reg.map_removed_get() == {"capacity": 0, "held": len(a), "collected_total": len(a), "lost_total": 0}
    boxes2, dead2 = cases["crowded"]
    assert not (dead & dead2).any()
    assert reg.map_delete_boxes(boxes2) == int(dead2.sum())
    assert MC.same_multiset(reg.map_removed_acquire(), a)
    reg.map_removed_set(BIG)  # on again with the capacity the buffer has: contents and totals stay
    assert reg.map_removed_get() == {"capacity": BIG, "held": len(a), "collected_total": len(a), "lost_total": 0}
    c = reg.map_removed_acquire(clear=True)
    assert MC.same_multiset(c, a)
    assert len(reg.map_removed_acquire()) == 0
    assert reg.map_removed_get() == {"capacity": BIG, "held": 0, "collected_total": len(a), "lost_total": 0}
    boxes3 = np.array([[6.0, 0.0, 0.0, 12.5, 9.5, 5.0]], np.float32)
    dead3 = MC.in_boxes(pts, boxes3)
    assert not ((dead | dead2) & dead3).any() and dead3.sum() > 50
    reg.map_delete_boxes(boxes3)
    assert MC.same_multiset(reg.map_removed_acquire(), pts[dead3])
    reg.map_removed_set(BIG // 2)  # another capacity: a new, empty buffer, totals zero
    assert reg.map_removed_get() == {"capacity": BIG // 2, "held": 0, "collected_total": 0, "lost_total": 0}
    assert MC.same_multiset(np.concatenate([reg.global_map(), pts[dead | dead2 | dead3]]), pts)
    reg.close()


# --------------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case", MC.CASES)
def test_delete_boxes_collects_exactly_what_it_removes(small_world, case):
    pts, cases = MC.world(small_world)
    boxes, dead = cases[case]
    reg = _registrar()
    reg.map_build(pts)
    reg.map_removed_set(BIG)
    before = reg.map_download()
    assert MC.same_multiset(before, pts)
    n_deleted = reg.map_delete_boxes(boxes)
    got = reg.map_removed_acquire()
    after = reg.map_download()
    info = reg.map_removed_get()
    print(f"{case}: {len(boxes)} boxes, expected {int(dead.sum())}, n_deleted {n_deleted}, held {info['held']}, map {len(before)} -> {len(after)}")
    assert n_deleted == int(dead.sum()) == info["held"] == len(got)
    assert MC.same_multiset(got, pts[dead])
    assert MC.same_multiset(np.concatenate([after, got]), before)
    assert info == {"capacity": BIG, "held": n_deleted, "collected_total": n_deleted, "lost_total": 0}
    reg.close()


# --------------------------------------------------------------------------------------------------------------------------- 2
def _one_scan(reg, S, mode, k, st, separate):
    """Scan k of local_map_cases' stream through `mode`, map_update = 0; separate: propagate and lii_local_map_segment first (stand-alone)"""
    kw = dict(leaf=LEAF, max_iterations=MAX_IT, scan_sorted=True, map_update=False, scan_dev=reg.device_scan(S.scans[k]))
    gs, as_ = np.full(3, 0.1), np.full(3, 0.1)
    if mode == "register":
        prop = reg.propagate_cv(S.PERIOD, gs, as_, st)
        if separate:
            reg.local_map_segment(prop.pos_end)
        out = prop.copy()
        reg.scan_register(out, prop, cv=True, **kw)
        return out
    if mode == "cv":
        if separate:
            reg.local_map_segment(reg.propagate_cv(S.PERIOD, gs, as_, st).pos_end)
        return reg.register_cv(S.PERIOD, gs, as_, st.copy(), **kw)[0]
    rows = S.imu_rows(k)
    return reg.register_imu(rows, S.t_beg(k), st.copy(), imu_en=True, **kw)[0]


@pytest.mark.parametrize("mode,separate", [("register", False), ("cv", False), ("imu", False), ("cv", True)])
def test_local_map_traverse_collects_every_move(mode, separate):
    """Per scan: map before = map after + what was newly collected; the new points lie in info.boxes, no point of the map after does;
    held grows by last_n_deleted; over the traverse collected_total == deleted_total.  The in-job handles never clear (the buffer grows),
    the stand-alone one acquires and clears at every scan."""
    S = _stream()
    reg = _registrar(max_map_points=400_000, filter_size_map=0.25)
    reg.map_build(S.map_pts)
    reg.local_map_set(CUBE_LEN, DET_RANGE, enabled=not separate)
    reg.map_removed_set(len(S.map_pts))
    if mode == "imu":
        reg.set_imu_noise(cov_gyr=0.1, cov_acc=0.1, mean_acc_norm=9.81)
        reg.imu_carry = S.carry0
    st = S.state0.copy()
    if mode != "imu":
        S.lo_rates(st)
    before = reg.map_download()
    hist = np.zeros((0, 3), np.float32)
    held, moves, two_axes = 0, 0, 0
    for k in range(S.n_scans):
        st = _one_scan(reg, S, mode, k, st, separate)
        if mode != "imu":
            S.lo_rates(st)
        info = reg.local_map_get()
        rinfo = reg.map_removed_get()
        after = reg.map_download()
        dead = MC.in_boxes(before, info["boxes"]) if info["n_boxes"] else np.zeros(len(before), bool)
        new = before[dead]
        print(f"{mode}{' stand-alone' if separate else ''} scan {k}: boxes {info['n_boxes']} deleted {info['n_deleted']} held {rinfo['held']} map {len(before)} -> {len(after)}")
        assert info["n_deleted"] == len(new), k
        assert rinfo["held"] - held == info["n_deleted"], k
        assert MC.same_multiset(after, before[~dead]), k
        if info["n_boxes"]:
            assert not MC.in_boxes(after, info["boxes"]).any(), k
        got = reg.map_removed_acquire(clear=separate)
        if separate:
            assert MC.same_multiset(got, new), k
            assert reg.map_removed_get()["held"] == 0
            held = 0
        else:
            hist = np.concatenate([hist, new])
            assert MC.same_multiset(got, hist), k
            held = rinfo["held"]
        assert MC.same_multiset(np.concatenate([after, new]), before), k
        assert MC.in_boxes(new, info["boxes"]).all() if len(new) else True
        moves += info["n_boxes"] > 0
        two_axes += info["n_boxes"] == 2
        before = after
    info, rinfo = reg.local_map_get(), reg.map_removed_get()
    assert moves >= 3 and two_axes >= 1 and info["deleted_total"] > 1000
    assert rinfo["collected_total"] == info["deleted_total"] and rinfo["lost_total"] == 0
    if not separate:
        assert MC.same_multiset(reg.global_map(), S.map_pts)  # history + live map: everything the run has mapped
    reg.close()


# --------------------------------------------------------------------------------------------------------------------------- 3
def test_overflow_keeps_the_map_and_what_was_held(small_world):
    pts, cases = MC.world(small_world)
    boxes, dead = cases["swallow"]
    R = int(dead.sum())
    cap = (R // 2) | 1
    assert 64 < cap < R and cap % 64 != 0
    reg = _registrar()
    reg.map_build(pts)
    reg.map_removed_set(cap)
    assert reg.map_delete_boxes(boxes) == R  # the delete completes
    info = reg.map_removed_get()
    print(f"overflow: removed {R}, capacity {cap}, held {info['held']}, lost {info['lost_total']}")
    assert info == {"capacity": cap, "held": cap, "collected_total": cap, "lost_total": R - cap}
    assert MC.same_multiset(reg.map_download(), pts[~dead])  # the map as with a large buffer (test 1)
    n = C.c_int32(0)
    assert reg.L.lii_map_removed_acquire(reg.h, None, 0, C.byref(n), 1) == CAPACITY and n.value == cap  # (the count; clears nothing)
    rc, got, n_got = _raw_acquire(reg, cap, clear=False)
    assert rc == CAPACITY and n_got == cap and not np.isnan(got).any()
    want = collections.Counter(map(bytes, MC.rows_sorted(pts[dead])))
    have = collections.Counter(map(bytes, MC.rows_sorted(got)))
    assert not have - want, "a stored point that was not removed, or one stored more often than it was removed"
    p, nv = C.c_void_p(), C.c_int32(0)
    assert reg.L.lii_map_removed_view(reg.h, C.byref(p), C.byref(nv)) == CAPACITY and nv.value == cap and p.value
    with pytest.raises(Exception) as e:
        reg.map_removed_acquire(clear=True)  # (strict: raises before anything is cleared)
    assert e.value.code == CAPACITY and reg.map_removed_get()["held"] == cap
    rc, got2, _ = _raw_acquire(reg, cap, clear=True)  # delivers and clears; still reports the overflow
    assert rc == CAPACITY and MC.same_multiset(got2, got)
    assert reg.map_removed_get() == {"capacity": cap, "held": 0, "collected_total": cap, "lost_total": R - cap}
    # the next delete collects again
    boxes2 = np.array([[8.0, -9.5, -2.0, 12.5, -7.5, 5.0]], np.float32)
    dead2 = MC.in_boxes(pts, boxes2)
    assert not (dead & dead2).any() and 0 < int(dead2.sum()) < cap
    assert reg.map_delete_boxes(boxes2) == int(dead2.sum())
    rc, got3, _ = _raw_acquire(reg, cap, clear=False)
    assert rc == 0 and MC.same_multiset(got3, pts[dead2])
    assert reg.map_removed_get() == {"capacity": cap, "held": len(got3), "collected_total": cap + len(got3), "lost_total": R - cap}
    reg.close()


def test_overflow_in_a_cube_move():
    """The same rule on the moving local map's strided squeeze: a move that removes more than the buffer holds."""
    S = _stream()
    cap = 1001
    reg = _registrar(max_map_points=400_000, filter_size_map=0.25)
    reg.map_build(S.map_pts)
    reg.local_map_set(CUBE_LEN, DET_RANGE, enabled=False)
    reg.map_removed_set(cap)
    before = reg.map_download()
    assert reg.local_map_segment([0.0, 0.0, 0.0])["n_boxes"] == 0
    info = reg.local_map_segment([6.0, 6.0, 0.0])  # trips x and y: two overlapping boxes
    dead = MC.in_boxes(before, info["boxes"])
    R = int(dead.sum())
    rinfo = reg.map_removed_get()
    print(f"cube move: {info['n_boxes']} boxes removed {info['n_deleted']} (expected {R}), capacity {cap}, held {rinfo['held']}, lost {rinfo['lost_total']}")
    assert info["n_boxes"] == 2 and info["n_deleted"] == R > cap and cap % 64 != 0
    assert rinfo == {"capacity": cap, "held": cap, "collected_total": cap, "lost_total": R - cap}
    assert MC.same_multiset(reg.map_download(), before[~dead])
    rc, got, n_got = _raw_acquire(reg, cap, clear=True)
    assert rc == CAPACITY and n_got == cap
    want = collections.Counter(map(bytes, MC.rows_sorted(before[dead])))
    have = collections.Counter(map(bytes, MC.rows_sorted(got)))
    assert not have - want
    assert reg.map_removed_get() == {"capacity": cap, "held": 0, "collected_total": cap, "lost_total": R - cap}
    reg.close()


# --------------------------------------------------------------------------------------------------------------------------- 4
def test_what_must_not_collect(small_world):
    import lidar_imu_init_amd as lii
    pts, cases = MC.world(small_world)
    boxes, dead = cases["crowded"]
    rng = np.random.default_rng(3)
    for env in (None, "force_rebuild"):
        old = os.environ.get("LII_TEST")
        if env:
            os.environ["LII_TEST"] = env  # every in-place update rebuilds the index first
        try:
            reg = _registrar()
        finally:
            os.environ.pop("LII_TEST", None)
            if old is not None:
                os.environ["LII_TEST"] = old
        reg.map_build(pts)
        reg.map_removed_set(BIG)
        assert reg.map_delete_boxes(boxes) == int(dead.sum())
        held = reg.map_removed_get()["held"]
        assert held == int(dead.sum()) > 0
        kept = reg.map_removed_acquire()
        live = pts[~dead]
        # Add_Points with down-sampling onto occupied voxels: the voxel centres themselves replace what the voxels hold
        ds = np.float32(MC.FILTER_SIZE_MAP)
        centres = (np.floor(live[rng.choice(len(live), 1500, replace=False)] / ds) * ds + ds / 2).astype(np.float32)
        n0 = reg.map_size()
        assert reg.map_add_points(centres, True) > 0
        replaced = n0 + len(np.unique(centres, axis=0)) - reg.map_size()
        assert replaced > 100, replaced  # points did leave the map - by down-sampling
        assert reg.map_removed_get()["held"] == held
        # lii_map_incremental
        q = (live[rng.choice(len(live), 3000, replace=False)] + rng.normal(0, 0.05, (3000, 3))).astype(np.float32)
        reg.scan_upload(np.c_[q, np.zeros(len(q), np.float32)])
        reg.downsample_skip()
        reg.iekf_iterate(lii.State(), True, False)
        m0 = MC.rows_sorted(reg.map_download())
        reg.map_incremental(lii.State())
        m1 = MC.rows_sorted(reg.map_download())
        assert m0.shape != m1.shape or not np.array_equal(m0, m1)  # (the map did change)
        assert reg.map_removed_get()["held"] == held
        # reset, build
        reg.map_reset()
        assert reg.map_removed_get()["held"] == held
        reg.map_build(pts)
        assert reg.map_removed_get()["held"] == held
        assert MC.same_multiset(reg.map_removed_acquire(), kept)  # ... and nothing touched the buffer
        assert reg.map_removed_get() == {"capacity": BIG, "held": held, "collected_total": held, "lost_total": 0}
        reg.close()


# --------------------------------------------------------------------------------------------------------------------------- 6
def test_off_is_off():
    """A handle that never heard of the order, one whose order is off again, one with the order on: the same states, the same map and
    the same launches per kind (lii_set_profiling(h, 3)) over scans that move the cube once - nothing rides in a launch of its own."""
    S = _stream()
    regs = [_registrar(max_map_points=400_000, filter_size_map=0.25) for _ in range(3)]
    regs[1].map_removed_set(1000)
    regs[1].map_removed_set(0)
    regs[2].map_removed_set(len(S.map_pts))
    st = []
    for r in regs:
        r.map_build(S.map_pts)
        r.local_map_set(CUBE_LEN, DET_RANGE, enabled=True)
        r.set_profiling(1)
        r.set_profiling(3)
        s = S.state0.copy()
        S.lo_rates(s)
        st.append(s)
    n_scans = 6
    gs, as_ = np.full(3, 0.1), np.full(3, 0.1)
    for k in range(n_scans):
        for i, r in enumerate(regs):
            st[i] = r.register_cv(S.PERIOD, gs, as_, st[i].copy(), leaf=LEAF, max_iterations=MAX_IT, scan_sorted=True, map_update=True,
                                  scan_dev=r.device_scan(S.scans[k]))[0]
            S.lo_rates(st[i])
        assert np.array_equal(st[0].pod.view(np.uint64), st[1].pod.view(np.uint64)) and np.array_equal(st[0].pod.view(np.uint64), st[2].pod.view(np.uint64)), k
    maps = [r.map_download() for r in regs]
    assert MC.same_multiset(maps[0], maps[1]) and MC.same_multiset(maps[0], maps[2])
    kinds = []
    for r in regs:
        kp, scans = r.kernel_profile()
        assert scans == n_scans
        kinds.append({k: v[1] for k, v in kp.items()})
        print("launches by kind:", kinds[-1])
    assert kinds[0] == kinds[1] == kinds[2]
    infos = [r.local_map_get() for r in regs]
    assert infos[0]["moves"] >= 1 and infos[0]["deleted_total"] > 0
    assert all(i["deleted_total"] == infos[0]["deleted_total"] for i in infos)
    assert regs[1].map_removed_get() == {"capacity": 0, "held": 0, "collected_total": 0, "lost_total": 0}
    assert regs[2].map_removed_get()["held"] == infos[2]["deleted_total"]
    for r in regs:
        r.close()


# --------------------------------------------------------------------------------------------------------------------------- 7
def test_refusals(small_world):
    from lidar_imu_init_amd import api
    S = _stream()
    reg = _registrar(max_map_points=400_000, filter_size_map=0.25)
    L, h = reg.L, reg.h
    n, p = C.c_int32(0), C.c_void_p()
    info = api.lii_map_removed_info(C.sizeof(api.lii_map_removed_info))
    buf = np.zeros((4, 3), np.float32)
    # before any lii_map_removed_set
    assert L.lii_map_removed_get(h, C.byref(info)) == STATE
    assert L.lii_map_removed_acquire(h, buf.ctypes.data_as(C.c_void_p), 4, C.byref(n), 0) == STATE
    assert L.lii_map_removed_view(h, C.byref(p), C.byref(n)) == STATE
    assert L.lii_map_removed_set(h, -1) == INVALID
    assert L.lii_map_removed_get(h, C.byref(info)) == STATE  # (a refused order is no order)
    reg.map_removed_set(1000)
    assert L.lii_map_removed_set(h, -5) == INVALID and reg.map_removed_get()["capacity"] == 1000
    assert L.lii_map_removed_get(h, None) == INVALID
    bad = api.lii_map_removed_info(8)
    assert L.lii_map_removed_get(h, C.byref(bad)) == INVALID
    assert L.lii_map_removed_acquire(h, buf.ctypes.data_as(C.c_void_p), 4, None, 0) == INVALID
    assert L.lii_map_removed_view(h, None, C.byref(n)) == INVALID
    assert L.lii_map_removed_view(h, C.byref(p), None) == INVALID
    # from inside lii_scan_job::while_waiting
    reg.map_build(S.map_pts)
    st = S.state0.copy()
    S.lo_rates(st)
    seen = []

    def hook():
        seen.append((L.lii_map_removed_set(h, 2000), L.lii_map_removed_get(h, C.byref(info)),
                     L.lii_map_removed_acquire(h, None, 0, C.byref(n), 0), L.lii_map_removed_view(h, C.byref(p), C.byref(n))))

    reg.register_cv(S.PERIOD, np.full(3, 0.1), np.full(3, 0.1), st.copy(), leaf=LEAF, max_iterations=MAX_IT, scan_sorted=True,
                    scan_dev=reg.device_scan(S.scans[0]), while_waiting=hook)
    assert seen == [(STATE, STATE, STATE, STATE)]
    assert reg.map_removed_get() == {"capacity": 1000, "held": 0, "collected_total": 0, "lost_total": 0}
    # a communicator attached: the order works where lii_map_delete_boxes does
    reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")
    box = np.array([[-5.0, -5.0, -5.0, 5.0, 5.0, 5.0]], np.float32)
    want = int(MC.in_boxes(S.map_pts, box).sum())
    reg.map_removed_set(want + 10)
    assert reg.map_delete_boxes(box) == want > 0
    assert MC.same_multiset(reg.map_removed_acquire(), np.asarray(S.map_pts, np.float32)[MC.in_boxes(S.map_pts, box)])
    reg.comm_destroy()
    reg.close()


# --------------------------------------------------------------------------------------------------------------------------- 8
def test_replay_host_global_map(tmp_path):
    """lii_replay_set_map_history places the order before the first scan; lii_replay_global_map = history + live map.  The stream's own
    cube (2 000 m) never moves, so the delete that fills the history is made through the host's handle behind the run."""
    import test_replay_host as T
    from lidar_imu_init_amd import api
    from lidar_imu_init_amd.api import lii_pc2_fields
    from harness import synth, wire
    d = T._drv()
    T._bind(d)
    d.lii_replay_set_local_map.argtypes = [C.c_void_p, C.c_int32]
    d.lii_replay_set_map_history.argtypes = [C.c_void_p, C.c_int32]
    d.lii_replay_global_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    d.lii_replay_handle.restype = C.c_void_p
    d.lii_replay_handle.argtypes = [C.c_void_p]
    (tmp_path / "config").mkdir()
    (tmp_path / "launch").mkdir()
    (tmp_path / "config" / "replay_test.yaml").write_text(T.YAML)
    (tmp_path / "launch" / "replay_test.launch").write_text(T.LAUNCH)
    launch = str(tmp_path / "launch" / "replay_test.launch")
    hall = synth.Hall(size=(24.0, 18.0, 6.0), n_boxes=8, seed=7)
    traj = synth.Trajectory()
    msg_period, n_msgs = 0.1, 8
    t_imu, gyro, accel = synth.simulate_imu(traj, -0.5, n_msgs * msg_period + 0.5, 200.0, np.eye(3), np.zeros(3), np.zeros(3), np.zeros(3), 0.0)
    fields = lii_pc2_fields(*wire.pc2_fields(wire.OUSTER))
    cfg = T.ReplayConfig(C.sizeof(T.ReplayConfig), 0, 40_000, 600_000, launch.encode(), None, None, 0, 0)
    rp = C.c_void_p()
    assert d.lii_replay_create(C.byref(cfg), C.byref(rp)) == 0
    n = C.c_int32(0)
    assert d.lii_replay_set_map_history(None, 10) == INVALID and d.lii_replay_set_map_history(rp, -1) == INVALID
    assert d.lii_replay_global_map(rp, None, 0, C.byref(n)) == STATE  # the switch is off
    assert d.lii_replay_set_local_map(rp, 1) == 0
    assert d.lii_replay_set_map_history(rp, 600_000) == 0
    k_imu = 0
    for k in range(n_msgs):
        stamp = k * msg_period
        scan = synth.make_distorted_scan(hall, "mid16k", traj, stamp, msg_period, noise=0.01, seed=3000 + k, blind=0.0)
        raw = np.frombuffer(wire.pack_pcl2(wire.OUSTER, scan[:, :3], np.zeros(len(scan), np.int32), scan[:, 3].astype(np.float64), stamp), np.uint8).copy()
        while k_imu < len(t_imu) and t_imu[k_imu] <= stamp + msg_period:
            g, a = np.ascontiguousarray(gyro[k_imu]), np.ascontiguousarray(accel[k_imu])
            assert d.lii_replay_imu(rp, float(t_imu[k_imu]), T._dp(g), T._dp(a)) == 0
            k_imu += 1
        assert d.lii_replay_pcl2(rp, stamp, raw.ctypes.data_as(C.c_void_p), len(scan), C.byref(fields)) == 0
        assert d.lii_replay_spin(rp) >= 0, d.lii_replay_last_error(rp)
    L = api.load_library()
    h = C.c_void_p(d.lii_replay_handle(rp))
    info = api.lii_map_removed_info(C.sizeof(api.lii_map_removed_info))
    assert L.lii_map_removed_get(h, C.byref(info)) == 0 and info.capacity == 600_000 and info.held == 0  # the order was placed; the cube never moved

    def fetch():
        assert d.lii_replay_global_map(rp, None, 0, C.byref(n)) == 0
        out = np.zeros((max(n.value, 1), 3), np.float32)
        assert d.lii_replay_global_map(rp, out.ctypes.data_as(C.c_void_p), n.value - 1, C.byref(n)) == CAPACITY
        assert d.lii_replay_global_map(rp, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)) == 0
        return out[:n.value]

    whole = fetch()
    assert len(whole) > 1000
    box = np.array([[0.0, -20.0, -5.0, 20.0, 20.0, 10.0]], np.float32)
    dead = MC.in_boxes(whole, box)
    nd = C.c_int32(0)
    assert L.lii_map_delete_boxes(h, box.ctypes.data_as(C.c_void_p), 1, C.byref(nd)) == 0 and nd.value == int(dead.sum()) > 100
    both = fetch()
    assert MC.same_multiset(both[:nd.value], whole[dead])        # the history comes first,
    assert MC.same_multiset(both[nd.value:], whole[~dead])       # the live map behind it
    assert MC.same_multiset(both, whole)
    d.lii_replay_destroy(rp)
