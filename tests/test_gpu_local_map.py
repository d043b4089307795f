"""The moving local map on the device: lii_local_map_set / _get / _segment and the in-job form of lii_scan_register, lii_scan_register_cv
and lii_scan_register_imu (lasermap_fov_segment, src/laserMapping.cpp:260-305, followed by the Delete_Point_Boxes call upstream never
made) against

  1. harness/fov_harness.py - the numpy restatement, float32 / float64 as the reference computes - bit for bit, and the UNMODIFIED
     reference tree's Delete_Point_Boxes (oracle/_ref, where it is built; the count by numpy otherwise);
  2. this library's separate calls: propagate, lii_local_map_segment, then the same registration on a second handle - the same device
     code on the same numbers, so every output is bit-equal;
  3. a traverse of new ground: under a map capacity that only a map that makes room survives, and against a host tree that follows it;
  4. itself with the feature off;
  5. the refusals of include/liinit_hip.h.

The traverse's set check keeps ONE host tree from the first scan to the end: the restatement's boxes go to it, and the same adds go to
it and to the device - map_incremental's decision made on the host from lii_neighbors_download and handed to lii_map_add_points and to
the tree's Add_Points, the route INTEGRATION.md section 2 names.  The tight-capacity run lets the job update the map itself."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from harness import fov_harness as F
from local_map_cases import CUBE_LEN, DET_RANGE, Stream, as_set, static_scan

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, STATE = -1, -4, -5
LEAF, MAX_IT = 0.25, 5
_cache = {}


def _stream():
    if "s" not in _cache:
        _cache["s"] = Stream()
    return _cache["s"]


def _registrar(**kw):
    import lidar_imu_init_amd as lii
    return lii.Registrar(**{**dict(max_scan_points=8_000, max_map_points=400_000, filter_size_map=0.25), **kw})


def _ref_tree(oracle, pts=None):
    if not oracle.ref_available():
        return None
    t = oracle.Tree("ref")
    if pts is not None:
        t.build(np.ascontiguousarray(pts, np.float32))
    return t


def _same_info(info, cube, boxes, tag):
    """cube, n_boxes and boxes of a lii_local_map_info against the restatement's float32 values, bit for bit"""
    assert info["initialized"] and cube.initialized, tag
    assert np.array_equal(info["cube"].view(np.uint32), cube.cube.view(np.uint32)), (tag, info["cube"], cube.cube)
    assert info["n_boxes"] == len(boxes), (tag, info["n_boxes"], len(boxes))
    assert np.array_equal(info["boxes"].view(np.uint32), np.ascontiguousarray(boxes, np.float32).view(np.uint32)), (tag, info["boxes"], boxes)
    assert info["moves"] == cube.moves, tag


# --------------------------------------------------------------------------------------------------------------------------- 1
def _script():
    pos = [[float(x), 0.0, 0.0] for x in range(0, 31)]  # +x in 1 m steps to 30 (the first call initialises)
    pos.append([35.0, 5.0, 0.0])                          # trips x and y in one call
    pos.append([40.0, 10.0, 5.0])                         # ... and all three axes
    pos += [[float(x), 10.0, 5.0] for x in range(39, 24, -1)]  # back along -x
    pos.append([13.0, 10.0, 5.0])                         # one jump of 12 m
    return np.array(pos)


def _face_points(rng):
    """points exactly on the faces of the boxes the restatement predicts for the first three moves of the script"""
    cube = F.LocalMapCube(CUBE_LEN, DET_RANGE)
    out, moves = [], 0
    for p in _script():
        for b in cube.segment(p):
            for a in range(3):
                for face in (b[a], b[3 + a]):
                    q = rng.uniform(b[:3], b[3:], (20, 3)).astype(np.float32)
                    q[:, a] = face
                    out.append(q)
        moves = cube.moves
        if moves == 3:
            break
    assert moves == 3
    return np.concatenate(out)


def test_standalone_call_against_restatement_and_reference_tree(oracle):
    rng = np.random.default_rng(5)
    base = rng.uniform([-25, -25, -3], [60, 25, 3], (30_000, 3)).astype(np.float32)
    faces = _face_points(rng)
    pts = as_set(np.concatenate([base, faces]))
    reg = _registrar(max_scan_points=8_000, max_map_points=60_000)
    # a call with no map: the cube is initialised, nothing else happens
    reg.local_map_set(CUBE_LEN, DET_RANGE, enabled=False)
    info = reg.local_map_segment([1.0, 2.0, 3.0])
    assert info["initialized"] and info["n_boxes"] == 0 and info["n_deleted"] == 0 and info["moves"] == 0
    assert np.array_equal(info["cube"], np.array([-19, -18, -17, 21, 22, 23], np.float32))
    info = reg.local_map_segment([7.0, 2.0, 3.0])  # ... or moved, with nothing to delete
    assert info["n_boxes"] == 1 and info["n_deleted"] == 0 and info["moves"] == 1 and reg.map_size() == 0
    reg.map_build(pts)
    reg.local_map_set(CUBE_LEN, DET_RANGE, enabled=False)  # Localmap_Initialized = false
    assert not reg.local_map_get()["initialized"]
    tree = _ref_tree(oracle, pts)
    cube = F.LocalMapCube(CUBE_LEN, DET_RANGE)
    live = pts
    script = _script()
    checkpoints = set(np.linspace(5, len(script) - 1, 6).astype(int).tolist())
    two, three, total = 0, 0, 0
    for i, p in enumerate(script):
        boxes = cube.segment(p)
        info = reg.local_map_segment(p)
        _same_info(info, cube, boxes, f"call {i} at {p}")
        dead = F.in_boxes(live, boxes)
        want = int(dead.sum())
        if tree is not None and len(boxes):
            assert tree.delete_boxes(boxes) == want
        print(f"call {i} at {p}: {len(boxes)} boxes, deleted {info['n_deleted']} (expected {want}), cube {info['cube']}")
        assert info["n_deleted"] == want, (i, info["n_deleted"], want)
        live = live[~dead]
        total += want
        assert info["deleted_total"] == total
        two += len(boxes) == 2
        three += len(boxes) == 3
        if i in checkpoints:
            got = as_set(reg.map_download())
            assert np.array_equal(got, as_set(live)), i
            if tree is not None:
                assert np.array_equal(got, as_set(tree.flatten())), i
            assert reg.map_size() == len(live)
    assert two >= 1 and three >= 1 and cube.moves >= 12 and total > 5_000
    # the face points of the first three moves: lower faces went, upper faces stayed - part of `live` above; here by count
    assert len(live) < len(pts)
    # ... and the index over what is left answers like the tree
    q = np.concatenate([live[rng.choice(len(live), 3000)] + rng.normal(0, 0.2, (3000, 3)), rng.uniform([-30, -30, -5], [65, 30, 5], (1000, 3))]).astype(np.float32)
    gp, gd, gc = reg.map_nearest(q, k=5, max_dist=5.0)
    if tree is not None:
        tp, td, tc = tree.knn(q, k=5, max_dist=5.0, threads=3)
        rows = np.arange(5)[None, :] < tc[:, None]
        assert np.array_equal(gc, tc)
        assert np.array_equal(np.where(rows, gd, 0).view(np.uint32), np.where(rows, td, 0).view(np.uint32))
        d = np.where(rows, td, np.inf)
        tied = ((d[:, :-1] == d[:, 1:]) & np.isfinite(d[:, 1:])).any(axis=1)  # (two equal d2 inside a list: either point may come first)
        assert tied.mean() < 0.01 and np.array_equal(gp[~tied], tp[~tied])
        tree.close()
    else:
        from map_nearest_cases import Brute, check_answer
        check_answer(Brute(q, live, keep=6, d2_max=5.0), 5, 5.0, gp, gd, gc, "lii_map_nearest after the moves")
    reg.close()


# --------------------------------------------------------------------------------------------------------------------------- 2
def _one_scan(reg, S, mode, k, st, map_update, separate):
    """Scan k of the stream through `mode` on `reg`; separate: propagate, lii_local_map_segment at the propagated pos_end, then the same
    registration.  Returns (state, report, propagated pos_end or None)."""
    scan = S.scans[k]
    kw = dict(leaf=LEAF, max_iterations=MAX_IT, scan_sorted=True, map_update=map_update, scan_dev=reg.device_scan(scan))
    gs, as_ = np.full(3, 0.1), np.full(3, 0.1)
    if mode == "register":
        prop = reg.propagate_cv(S.PERIOD, gs, as_, st)
        if separate:
            reg.local_map_segment(prop.pos_end)
        out = prop.copy()
        rep = reg.scan_register(out, prop, cv=True, **kw)
        return out, rep
    if mode == "cv":
        if separate:
            reg.local_map_segment(reg.propagate_cv(S.PERIOD, gs, as_, st).pos_end)
        out, _, rep = reg.register_cv(S.PERIOD, gs, as_, st.copy(), **kw)
        return out, rep
    rows = S.imu_rows(k)
    if separate:
        carry = reg.imu_carry
        prop, _ = reg.propagate_imu(rows, S.t_beg(k), S.t_end(k), st)
        reg.imu_carry = carry  # (the registration below propagates again, from the same carry)
        reg.local_map_segment(prop.pos_end)
    out, _, rep = reg.register_imu(rows, S.t_beg(k), st.copy(), imu_en=True, **kw)
    return out, rep


@pytest.mark.parametrize("map_update", [True, False])
@pytest.mark.parametrize("mode", ["register", "cv", "imu"])
def test_in_job_equals_separate_calls(mode, map_update):
    S = _stream()
    regs = [_registrar(), _registrar()]
    for r, on in zip(regs, (True, False)):
        r.map_build(S.map_pts)
        r.local_map_set(CUBE_LEN, DET_RANGE, enabled=on)
        if mode == "imu":
            r.set_imu_noise(cov_gyr=0.1, cov_acc=0.1, mean_acc_norm=9.81)
            r.imu_carry = S.carry0
    st = [S.state0.copy(), S.state0.copy()]
    if mode != "imu":
        for s in st:
            S.lo_rates(s)
    moved, two_axes, deleted = 0, 0, 0
    for k in range(S.n_scans):
        outs = []
        for i in range(2):
            st[i], rep = _one_scan(regs[i], S, mode, k, st[i], map_update, separate=(i == 1))
            n = len(regs[i].scan_download(1))
            outs.append((rep, regs[i].neighbors(n), regs[i].local_map_get()))
            if mode != "imu":
                S.lo_rates(st[i])
        (ra, na, ia), (rb, nb, ib) = outs
        print(f"{mode} scan {k}: effect {ra['effect_num']} / {rb['effect_num']}  iterations {ra['iterations']}  boxes {ia['n_boxes']}  deleted {ia['n_deleted']}  "
              f"cube {ia['cube']}  pos {st[0].pos_end}")
        assert np.array_equal(st[0].pod.view(np.uint64), st[1].pod.view(np.uint64)), k
        for key in ("iterations", "searches", "effect_num", "converged"):
            assert ra[key] == rb[key], (k, key)
        assert np.array_equal(ra["normal_eq"].view(np.uint64), rb["normal_eq"].view(np.uint64)), k
        for a, b in zip(na, nb):
            assert np.array_equal(a, b), k
        for key in ("initialized", "n_boxes", "n_deleted", "moves", "deleted_total"):
            assert ia[key] == ib[key], (k, key, ia[key], ib[key])
        assert np.array_equal(ia["cube"].view(np.uint32), ib["cube"].view(np.uint32)) and np.array_equal(ia["boxes"].view(np.uint32), ib["boxes"].view(np.uint32)), k
        assert ra["effect_num"] > 100, (k, ra)
        moved += ia["n_boxes"] > 0
        two_axes += ia["n_boxes"] == 2
        deleted += ia["n_deleted"]
        assert ia["moves"] == moved
    assert moved >= 3 and two_axes >= 1 and deleted > 0, (moved, two_axes, deleted)
    got = [as_set(r.map_download()) for r in regs]
    assert np.array_equal(got[0], got[1])
    assert regs[0].map_size() == regs[1].map_size() == len(got[0])
    for r in regs:
        r.close()


# --------------------------------------------------------------------------------------------------------------------------- 3
class _Corridor:
    """260 m of corridor, 12 m wide, pillars along both walls every 7 m (they hold the registration along the axis); the sensor sees 12 m:
    less than the 15 m it keeps from every face of the cube, so whatever it maps lies inside the cube and goes when the cube has passed."""
    STEP, RANGE = 2.5, 12.0

    def __init__(self):
        from harness import synth
        self.hall = synth.Hall(size=(260.0, 12.0, 6.0), n_boxes=0, seed=1)
        lo_z = self.hall.lo[2]
        self.hall.boxes = []
        for i, x in enumerate(np.arange(-125.0, 126.0, 7.0)):
            y0 = 3.8 if i % 2 else -6.0
            self.hall.boxes.append((np.array([x, y0, lo_z]), np.array([x + 1.5, y0 + 2.2, lo_z + 4.0])))
        self.x0 = -120.0

    def pose(self, k):
        from harness import synth
        return synth.rot_zyx(0.0, 0.0, 0.02 * np.sin(0.3 * k)), np.array([self.x0 + self.STEP * k, 0.4 * np.sin(0.2 * k), 0.0])

    def scan(self, k):
        R, p = self.pose(k)
        return static_scan(self.hall, R, p, seed=70 + k, max_range=self.RANGE)

    def states(self, k):
        """(propagated state: the true pose a few centimetres off, the same for every handle)"""
        import lidar_imu_init_amd as lii
        from harness.lo_harness import so3_exp
        R, p = self.pose(k)
        st = lii.State()
        st.rot_end[:] = R @ so3_exp(np.array([0.002, -0.001, 0.003]))
        st.pos_end[:] = p + np.array([0.03, -0.02, 0.01])
        return st


def _corridor_scan(reg, W, k, map_update):
    prop = W.states(k)
    st = prop.copy()
    rep = reg.scan_register(st, prop, leaf=LEAF, max_iterations=MAX_IT, scan_sorted=True, map_update=map_update, scan_dev=reg.device_scan(W.scan(k)))
    return st, prop, rep


def test_traverse_of_new_ground_under_a_tight_capacity():
    import lidar_imu_init_amd as lii
    W = _Corridor()
    n_scans = int(225.0 / W.STEP)  # 225 m: 44 moves of 5 m behind the first
    # ---- the steady state of the cube's map, measured on the first laps: the map's size over the moves 3 .. 8
    reg = _registrar(max_map_points=400_000)
    reg.local_map_set(CUBE_LEN, DET_RANGE, enabled=True)
    sizes, k = [], 0
    first = W.states(0)
    reg.scan_upload(W.scan(0))
    reg.downsample(LEAF)
    assert reg.map_build_from_scan(first) > 1000  # (the first scan becomes the map, src/laserMapping.cpp:921-929)
    while True:
        k += 1
        _corridor_scan(reg, W, k, True)
        info = reg.local_map_get()
        if info["moves"] >= 3:
            sizes.append(reg.map_size())
        if info["moves"] >= 8:
            break
    reg.close()
    steady = max(sizes)
    cap = int(1.5 * steady)
    print(f"steady state of the cube's map: {steady} points over moves 3 .. 8 ({k} scans); max_map_points {cap}")

    def run(on):
        reg = _registrar(max_map_points=cap)
        try:
            return traverse(reg, on)
        finally:
            reg.close()

    def traverse(reg, on):
        if on:
            reg.local_map_set(CUBE_LEN, DET_RANGE, enabled=True)
        cube = F.LocalMapCube(CUBE_LEN, DET_RANGE)
        reg.scan_upload(W.scan(0))
        reg.downsample(LEAF)
        reg.map_build_from_scan(W.states(0))
        largest = 0
        for k in range(1, n_scans):
            boxes = cube.segment(W.states(k).pos_end)  # (lii_scan_register: the propagated state is the `state` argument)
            st, prop, rep = _corridor_scan(reg, W, k, True)
            assert rep["effect_num"] > 100, (k, rep)
            if on:
                _same_info(reg.local_map_get(), cube, boxes, f"scan {k}")
            n = reg.map_size()
            largest = max(largest, n)
            assert n <= cap
        return cube.moves, largest

    moves, largest = run(True)
    print(f"local map on: {moves} moves over {n_scans} scans, largest map {largest} of {cap}")
    assert moves >= 40
    with pytest.raises(lii.LIIError) as e:  # today's behaviour, the contrast: nothing makes room
        run(False)
    assert e.value.code == CAPACITY


def _world(body, st):
    """pointBodyToWorld (src/laserMapping.cpp:209-220) of the down-sampled cloud at state `st`, stored to float32"""
    b = np.asarray(body, np.float64)[:, :3]
    return ((b @ st.offset_R_L_I.T + st.offset_T_L_I) @ st.rot_end.T + st.pos_end).astype(np.float32)


def _d2(a, b):
    d = (a - b).astype(np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(np.float32)


def _host_map_incremental(world, nbr, cnt, fs):
    """map_incremental's decision (src/laserMapping.cpp:516-553) in numpy, from the world points and the neighbour lists the registration
    left: (PointToAdd, PointNoNeedDownsample).  Both sides of the replay get THESE lists, so it decides once for both."""
    mid = (np.floor(world.astype(np.float64) / fs) * fs + 0.5 * fs).astype(np.float32)
    dist = _d2(world, mid)
    has = cnt > 0
    nodown = has & np.all(np.abs(nbr[:, 0] - mid).astype(np.float64) > 0.5 * fs, axis=1)
    closer = (_d2(nbr, mid[:, None, :]) < dist[:, None]).any(axis=1) & (cnt >= 5)
    add = ~has | (~nodown & ~closer)
    return np.ascontiguousarray(world[add]), np.ascontiguousarray(world[nodown])


def test_traverse_equals_a_host_replay(oracle):
    """ONE host tree from the first scan to the end of the 44-move traverse - the unmodified reference tree where it is built, the
    restated one otherwise (rebuilt from the survivors at a move: it has no box delete of its own).  Per scan the device registers with
    the local map on and map_update off; the host tree gets the restatement's boxes, and BOTH get the same adds: map_incremental's decision
    made on the host from lii_neighbors_download, handed to lii_map_add_points and to the tree's Add_Points.  Counts agree at every
    scan, the sets at every tenth move and at the end."""
    W = _Corridor()
    n_scans = int(225.0 / W.STEP)
    fs = 0.25
    ref = oracle.ref_available()
    tree = oracle.Tree("ref" if ref else "oracle", downsample=fs)
    reg = _registrar(max_map_points=400_000, filter_size_map=fs)
    reg.local_map_set(CUBE_LEN, DET_RANGE, enabled=True)
    reg.scan_upload(W.scan(0))
    reg.downsample(LEAF)
    seed = _world(reg.scan_download(1), W.states(0))
    reg.map_build(seed)
    tree.build(seed)
    cube = F.LocalMapCube(CUBE_LEN, DET_RANGE)
    checked, deleted, added = 0, 0, 0
    for k in range(1, n_scans):
        boxes = cube.segment(W.states(k).pos_end)
        want = 0
        if len(boxes):
            if ref:
                want = tree.delete_boxes(boxes)
            else:
                now = tree.flatten()
                dead = F.in_boxes(now, boxes)
                want = int(dead.sum())
                tree.close()
                tree = oracle.Tree("oracle", downsample=fs)
                tree.build(now[~dead])
        st, prop, rep = _corridor_scan(reg, W, k, False)
        assert rep["effect_num"] > 100, (k, rep)
        info = reg.local_map_get()
        _same_info(info, cube, boxes, f"scan {k}")
        assert info["n_deleted"] == want, (k, info["n_deleted"], want)
        deleted += want
        body = reg.scan_download(1)
        nbr, cnt, _ = reg.neighbors(len(body))
        a, b = _host_map_incremental(_world(body, st), nbr, cnt, fs)
        assert reg.map_add_points(a, True) == tree.add_points(a, True), k
        reg.map_add_points(b, False)
        tree.add_points(b, False)
        added += len(a) + len(b)
        valid = tree.validnum()  # (-1: the reference tree's rebuild thread holds the lock just now, KD_TREE::validnum)
        assert valid in (-1, reg.map_size()), (k, valid)
        if (len(boxes) and cube.moves % 10 == 0) or k == n_scans - 1:
            for _ in range(400):  # (the reference tree reports its size only between two background rebuilds, and flatten sizes its buffer by it)
                if tree.size() >= 0 and tree.validnum() >= 0:
                    break
                time.sleep(0.005)
            got, host = as_set(reg.map_download()), as_set(tree.flatten())
            print(f"scan {k}, move {cube.moves}: device {len(got)} points, host tree {len(host)}")
            assert got.shape == host.shape and np.array_equal(got, host), k
            checked += 1
    print(f"{cube.moves} moves, {deleted} points deleted, {added} handed to Add_Points, {checked} set comparisons with the "
          f"{'reference' if ref else 'restated'} tree")
    assert cube.moves >= 40 and checked >= 5 and deleted > 10_000 and added > 10_000
    tree.close()
    reg.close()


# --------------------------------------------------------------------------------------------------------------------------- 4
LAUNCHES_PER_SCAN = 3  # k_local_map_tomb, k_cell_apply_listed, k_local_map_finish


def test_off_is_off():
    S = _stream()
    regs = [_registrar(), _registrar(), _registrar()]
    regs[1].local_map_set(CUBE_LEN, DET_RANGE, enabled=False)
    regs[2].local_map_set(4000.0, DET_RANGE, enabled=True)
    st = []
    for r in regs:
        r.map_build(S.map_pts)
        r.set_profiling(1)
        r.set_profiling(3)
        s = S.state0.copy()
        S.lo_rates(s)
        st.append(s)
    n_scans = 6
    for k in range(n_scans):
        for i, r in enumerate(regs):
            st[i], rep = _one_scan(r, S, "cv", k, st[i], True, separate=False)
            S.lo_rates(st[i])
        assert np.array_equal(st[0].pod.view(np.uint64), st[1].pod.view(np.uint64)) and np.array_equal(st[0].pod.view(np.uint64), st[2].pod.view(np.uint64)), k
    sets = [as_set(r.map_download()) for r in regs]
    assert np.array_equal(sets[0], sets[1]) and np.array_equal(sets[0], sets[2])
    counts = []
    for r in regs:
        kp, scans = r.kernel_profile()
        assert scans == n_scans
        counts.append(sum(v[1] for v in kp.values()))
        print("launches by kind:", {k: v[1] for k, v in kp.items()})
    info = regs[2].local_map_get()
    assert info["initialized"] and info["moves"] == 0 and info["deleted_total"] == 0
    assert counts[0] == counts[1]
    assert counts[2] - counts[0] == LAUNCHES_PER_SCAN * n_scans
    for r in regs:
        r.close()


# --------------------------------------------------------------------------------------------------------------------------- 5
def test_refusals():
    import lidar_imu_init_amd as lii
    from lidar_imu_init_amd import api
    S = _stream()
    reg = _registrar()
    L, h = reg.L, reg.h

    def code(fn, *a, **kw):
        try:
            fn(*a, **kw)
            return 0
        except lii.LIIError as e:
            return e.code

    info = api.lii_local_map_info()
    assert code(reg.local_map_segment, [0, 0, 0]) == STATE  # before lii_local_map_set
    assert code(reg.local_map_get) == STATE
    for cube_len, det in ((float("nan"), 10.0), (float("inf"), 10.0), (40.0, float("nan")), (40.0, float("inf")), (40.0, 0.0), (40.0, -1.0),
                          (30.0, 10.0), (29.0, 10.0), (200.0, 300.0)):
        assert code(reg.local_map_set, cube_len, det) == INVALID, (cube_len, det)
    assert code(reg.local_map_segment, [0, 0, 0]) == STATE  # (a refused setting is no setting)
    o = api.lii_local_map_opts(C.sizeof(api.lii_local_map_opts), 2, 40.0, 10.0, 0)
    assert L.lii_local_map_set(h, C.byref(o)) == INVALID
    o = api.lii_local_map_opts(8, 1, 40.0, 10.0, 0)
    assert L.lii_local_map_set(h, C.byref(o)) == INVALID
    assert L.lii_local_map_set(h, None) == INVALID
    reg.local_map_set(CUBE_LEN, DET_RANGE, enabled=False)
    assert L.lii_local_map_get(h, None) == INVALID
    assert L.lii_local_map_segment(h, None, C.byref(info)) == INVALID
    for bad in ([float("nan"), 0, 0], [0, float("inf"), 0], [0, 0, -float("inf")]):
        assert code(reg.local_map_segment, bad) == INVALID
    assert not reg.local_map_get()["initialized"]  # nothing changed
    # a refused lii_local_map_set leaves the previous setting in force: the cube of the 40 / 10 setting goes on
    reg.local_map_segment([0.0, 0.0, 0.0])
    assert code(reg.local_map_set, 20.0, 10.0) == INVALID
    info2 = reg.local_map_segment([5.0, 0.0, 0.0])
    assert info2["initialized"] and info2["n_boxes"] == 1 and np.array_equal(info2["cube"], np.array([-15, -20, -20, 25, 20, 20], np.float32))
    # enqueue only
    assert reg.local_map_segment([10.0, 0.0, 0.0], report=False) is None
    assert reg.local_map_get()["moves"] == 2
    # a communicator attached: single rank for now
    reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")
    assert code(reg.local_map_set, CUBE_LEN, DET_RANGE) == STATE
    assert code(reg.local_map_segment, [0, 0, 0]) == STATE
    reg.comm_destroy()
    reg.local_map_set(CUBE_LEN, DET_RANGE, enabled=True)
    reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")
    reg.map_build(S.map_pts)
    st = S.state0.copy()
    S.lo_rates(st)
    assert code(reg.scan_register, st.copy(), st, cv=True, leaf=LEAF, max_iterations=MAX_IT, scan_sorted=True, scan_dev=reg.device_scan(S.scans[0])) == STATE
    reg.comm_destroy()
    reg.close()
    # LII_TEST=host_solve: the in-job form is refused, the stand-alone call serves
    old = os.environ.get("LII_TEST")
    os.environ["LII_TEST"] = "host_solve"
    try:
        reg = _registrar()
    finally:
        os.environ.pop("LII_TEST", None)
        if old is not None:
            os.environ["LII_TEST"] = old
    reg.map_build(S.map_pts)
    reg.local_map_set(CUBE_LEN, DET_RANGE, enabled=True)
    assert code(reg.scan_register, st.copy(), st, cv=True, leaf=LEAF, max_iterations=MAX_IT, scan_sorted=True, scan_dev=reg.device_scan(S.scans[0])) == STATE
    assert reg.local_map_segment(st.pos_end)["initialized"]
    reg.local_map_set(CUBE_LEN, DET_RANGE, enabled=False)
    assert code(reg.scan_register, st.copy(), st, cv=True, leaf=LEAF, max_iterations=MAX_IT, scan_sorted=True, scan_dev=reg.device_scan(S.scans[0])) == 0
    reg.close()
