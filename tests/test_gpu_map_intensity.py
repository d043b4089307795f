"""Map points keep their intensity: lii_map_build_xyzi / lii_map_add_points_xyzi in, the _xyzi queries, the history and lii_map_pcd out.

Expected intensities never come from the library: every cloud has pairwise distinct (x, y, z) bit triples (asserted), and the expectation
for any returned row is a lookup of its triple in the inputs (map_intensity_cases.Table).  Every comparison is of float BITS.  Which
triples survive an update is pinned to the oracle and the reference tree by test_gpu_map.py / test_gpu_map_points.py; here every _xyzi
call must also return the xyz / d2 / counts / offsets bits of its 3-float sibling on the same map."""
import ctypes as C
import os

import numpy as np
import pytest

import map_intensity_cases as IC

pytestmark = pytest.mark.gpu

INVALID, STATE, CAPACITY = -1, -5, -4


def _registrar(env=None, **kw):
    import lidar_imu_init_amd as lii
    kw = {**dict(max_scan_points=20_000, max_map_points=100_000, filter_size_map=IC.DS), **kw}
    if env is None:
        return lii.Registrar(**kw)
    os.environ["LII_TEST"] = env
    try:
        return lii.Registrar(**kw)
    finally:
        del os.environ["LII_TEST"]


def _code(fn, *a, **kw):
    import lidar_imu_init_amd as lii
    try:
        fn(*a, **kw)
        return 0
    except lii.LIIError as e:
        return e.code


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _dev_array(reg, addr, shape, typestr):
    """device memory -> numpy, through the runtime the library itself uses"""
    hip = C.CDLL(reg.L._name)
    out = np.zeros(shape, np.dtype(typestr))
    reg.synchronize()
    if out.nbytes:
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(int(addr)), C.c_size_t(out.nbytes), C.c_int(2)) == 0  # hipMemcpyDeviceToHost
    return out


def _dev_filled(reg, a):
    addr = reg.dev_alloc(a.nbytes)
    reg.dev_upload(addr, a)
    return addr


def _assert_map_is(reg, want_xyzi, table):
    """The map is `want_xyzi` as a multiset of (x, y, z, intensity) rows; the 3-float download holds the same xyz; every row looks up."""
    got = reg.map_download_xyzi()
    table.check(got)
    assert IC.same_rows_as_set(got, want_xyzi), f"the map holds {len(got)} rows, expected {len(want_xyzi)}"
    assert IC.same_rows_as_set(reg.map_download(), got[:, :3]) and reg.map_size() == len(got)


# ------------------------------------------------------------------------------------------------ build and download
@pytest.fixture(scope="module")
def big_cloud():
    c = IC.distinct_cloud(np.random.default_rng(70), 70_000, lo=-40.0, hi=40.0)
    IC.assert_distinct_triples(c)
    assert len(c) > 65_536 + 1000  # crosses a 65 536-row staging chunk
    return c


@pytest.mark.parametrize("n", (1, 257, 70_000))
@pytest.mark.parametrize("layout", ("xyzi16", "xyzinormal48"))
def test_build_and_download(big_cloud, n, layout):
    cloud = big_cloud[:min(n, len(big_cloud))]
    table = IC.Table(cloud)
    reg = _registrar()
    reg.map_build_xyzi(cloud if layout == "xyzi16" else IC.as_xyzinormal(cloud))
    _assert_map_is(reg, cloud, table)
    # count only / capacity, as lii_map_download
    L, h = reg.L, reg.h
    cnt = C.c_int32(-1)
    assert L.lii_map_download_xyzi(h, None, 0, C.byref(cnt)) == 0 and cnt.value == len(cloud)
    small = np.full((max(len(cloud) - 1, 1), 4), 7.0, np.float32)
    if len(cloud) > 1:
        assert L.lii_map_download_xyzi(h, small.ctypes.data, len(cloud) - 1, C.byref(cnt)) == CAPACITY and (small == 7.0).all()
    reg.close()


def test_bad_offsets_are_refused_and_plain_builds_read_back_zero():
    rng = np.random.default_rng(71)
    cloud = IC.distinct_cloud(rng, 500)
    more = IC.distinct_cloud(rng, 100, lo=20, hi=30, first=1 + len(cloud))
    IC.assert_distinct_triples(cloud, more)
    reg = _registrar()
    reg.map_build_xyzi(cloud)
    L, h = reg.L, reg.h
    rec = IC.as_xyzinormal(more)
    n = C.c_int32(-1)
    # negative, not a multiple of 4, overlapping x / y / z, offset + 4 > stride; a stride without room for a fourth float
    for stride, off in ((48, -4), (48, 14), (48, 0), (48, 8), (48, 48), (48, 46), (16, 16), (12, 12), (16, 13)):
        assert L.lii_map_build_xyzi(h, rec.ctypes.data, len(rec), stride, off) == INVALID, (stride, off)
        assert L.lii_map_add_points_xyzi(h, rec.ctypes.data, len(rec), stride, off, 0, C.byref(n)) == INVALID, (stride, off)
    assert L.lii_map_build_xyzi(h, None, 3, 16, 12) == INVALID and L.lii_map_add_points_xyzi(h, None, 3, 16, 12, 1, None) == INVALID
    assert L.lii_map_build_xyzi(h, rec.ctypes.data, -1, 48, 32) == INVALID
    _assert_map_is(reg, cloud, IC.Table(cloud))  # the map is untouched
    # every aligned offset behind the coordinates is accepted: the word there is what is stored
    assert L.lii_map_add_points_xyzi(h, rec.ctypes.data, len(rec), 48, 44, 0, None) == 0
    got = reg.map_download_xyzi()
    assert len(got) == len(cloud) + len(more)
    new = got[got[:, 0] >= 15]  # (`more` lies in [20, 30), the map in [-10, 10))
    assert len(new) == len(more) and (new[:, 3] == np.float32(-7.5)).all()
    # points stored through the 3-float entry points carry 0.0f (all bits clear)
    reg.map_build(cloud[:, :3])
    got = reg.map_download_xyzi()
    assert IC.same_rows_as_set(got[:, :3], cloud[:, :3]) and (_bits(got[:, 3]) == 0).all()
    reg.map_add_points(more[:, :3], False)
    assert (_bits(reg.map_download_xyzi()[:, 3]) == 0).all()
    reg.close()


def test_nan_and_special_intensities_travel_bit_for_bit():
    rng = np.random.default_rng(72)
    cloud = IC.distinct_cloud(rng, 64)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x7FA00000, 0xFFFFFFFF], np.uint32)
    w = _bits(cloud[:, 3]).copy()
    w[:4], w[32:36] = special[:4], special[4:]  # quiet and signalling NaNs with payloads, infinities, -0, a denormal: in the build and in the batch
    cloud = np.ascontiguousarray(np.c_[_bits(cloud[:, :3]), w].astype(np.uint32).view(np.float32))
    assert len(np.unique(IC.voxel_of(cloud, IC.DS), axis=0)) == len(cloud)  # a voxel each: the fold keeps every point
    reg = _registrar()
    reg.map_build_xyzi(cloud[:32])
    assert reg.map_add_points_xyzi(cloud[32:], True) == 32
    got = reg.map_download_xyzi()
    IC.Table(cloud).check(got)
    assert IC.same_rows_as_set(got, cloud)
    reg.close()


# ------------------------------------------------------------------------------------------------ Add_Points with down-sampling: the sorted fold
def _plain_twin(case, **kw):
    """The same build and batch through the 3-float entry points, on a handle of its own: (events, map xyz)."""
    reg = _registrar(**kw)
    reg.map_build(case["stored"][:, :3])
    ev = reg.map_add_points(case["batch"][:, :3], True)
    got = reg.map_download()
    zeros = reg.map_download_xyzi()[:, 3]
    reg.close()
    return ev, got, zeros


@pytest.mark.parametrize("form", ("cells_2x2x2", "wide_walk"))
def test_fold_keeps_the_intensity_of_the_point_it_keeps(form):
    """Voxels with 1, 3, 8, 9 and 20 batch points (9 and 20 leave the eight-lane shuffle for the replay from memory), into an empty box, a
    box where the stored point wins, one where a batch point wins, boxes with several stored points.  wide_walk: a down-sample box of 1 m
    on a 0.3 m cell grid - the sequential walk of a box wider than 2 x 2 x 2 cells."""
    kw = {} if form == "cells_2x2x2" else dict(filter_size_map=1.0, map_cell_size=0.3)
    case = IC.fold_case(seed=5 if form == "cells_2x2x2" else 6, ds=kw.get("filter_size_map", IC.DS))
    IC.check_fold_case(case)
    table = IC.Table(case["stored"], case["batch"])
    reg = _registrar(**kw)
    reg.map_build_xyzi(case["stored"])
    events = reg.map_add_points_xyzi(case["batch"], True)
    _assert_map_is(reg, case["survivors"], table)
    ev3, xyz3, zeros = _plain_twin(case, **kw)
    assert events == ev3 and IC.same_rows_as_set(xyz3, case["survivors"][:, :3]) and (_bits(zeros) == 0).all()
    # the same batch as 48-byte records into a map that was built without intensities: stored winners keep 0.0f, batch winners bring theirs
    reg.map_build(case["stored"][:, :3])
    assert reg.map_add_points_xyzi(IC.as_xyzinormal(case["batch"]), True) == events
    got = reg.map_download_xyzi()
    assert IC.same_rows_as_set(got[:, :3], case["survivors"][:, :3])
    from_batch = np.isin(_bits(got[:, 3]), _bits(case["batch"][:, 3]))
    IC.Table(case["batch"]).check(got[from_batch])
    assert (_bits(got[~from_batch, 3]) == 0).all()
    assert int(from_batch.sum()) == int(np.isin(_bits(case["survivors"][:, 3]), _bits(case["batch"][:, 3])).sum())
    reg.close()


def test_fold_into_an_empty_map():
    case = IC.fold_case(seed=8)
    batch = case["batch"]
    d2, vox = IC.centre_d2(batch, IC.DS), IC.voxel_of(batch, IC.DS)
    keep = np.zeros(len(batch), bool)
    for v in {tuple(v) for v in vox}:
        m = np.flatnonzero((vox == np.array(v)).all(axis=1))
        keep[m[np.argmin(d2[m])]] = True
    reg = _registrar()
    reg.map_reset()
    reg.map_add_points_xyzi(batch, True)
    _assert_map_is(reg, batch[keep], IC.Table(batch))
    reg.close()


# ------------------------------------------------------------------------------------------------ growth and recovery
@pytest.mark.parametrize("env", (None, "map_tight", "force_rebuild"))
@pytest.mark.parametrize("n_batches", (1, 5))
def test_cell_that_outgrows_its_slack_keeps_every_intensity(env, n_batches):
    """40 inserts without down-sampling into ONE grid cell, in one batch and over five: the cell outgrows its slack and moves to the tail.
    map_tight: no spare room is provisioned - inserts are parked and re-inserted by the rebuild; force_rebuild: a garbage collection in
    front of every update.  Nothing may come back as zero."""
    rng = np.random.default_rng(73)
    base = IC.distinct_cloud(rng, 2000)
    grow = IC.growth_batches()
    IC.check_growth_batches(grow)
    far = IC.with_intensity((rng.uniform(-1, 1, (300, 3)) * 300 + np.array([4000.0, 0, 0])).astype(np.float32), first=5000)  # every point a new block
    IC.assert_distinct_triples(base, grow, far)
    table = IC.Table(base, grow, far)
    reg = _registrar(env=env)
    reg.map_build_xyzi(base)
    for part in np.array_split(grow, n_batches):
        assert reg.map_add_points_xyzi(part, False) == 0
    reg.map_add_points_xyzi(far, False)
    want = np.concatenate([base, grow, far])
    _assert_map_is(reg, want, table)
    assert (reg.map_download_xyzi()[:, 3] != 0).all()
    reg.close()


# ------------------------------------------------------------------------------------------------ deletes and history
def _in_boxes(p, boxes):
    p = np.ascontiguousarray(p, np.float32)[:, :3]
    m = np.zeros(len(p), bool)
    for b in np.ascontiguousarray(boxes, np.float32).reshape(-1, 6):
        m |= ((b[:3] <= p) & (p < b[3:])).all(axis=1)
    return m


def test_deletes_hand_the_victims_intensities_to_the_history():
    rng = np.random.default_rng(74)
    xyz = np.unique(rng.uniform([-19.0, -4.0, -4.0], [19.0, 4.0, 4.0], (4000, 3)).astype(np.float32), axis=0)  # a slab along x: dense enough for the boxes to overlap on points
    cloud = IC.with_intensity(xyz[(xyz != 0).all(axis=1)][rng.permutation(len(xyz))])
    IC.assert_distinct_triples(cloud)
    table = IC.Table(cloud)
    reg = _registrar()
    reg.map_build_xyzi(cloud)
    reg.map_removed_set(len(cloud))
    # by box (a point in two boxes goes once)
    boxes = np.array([[-3, -3, -3, 3, 3, 3], [1, 1, 1, 6, 6, 6], [50, 50, 50, 60, 60, 60]], np.float32)
    dead = _in_boxes(cloud, boxes)
    assert dead.sum() > 20 and (_in_boxes(cloud, boxes[:1]) & _in_boxes(cloud, boxes[1:2])).sum() > 0
    assert reg.map_delete_boxes(boxes) == int(dead.sum())
    hist = reg.map_removed_acquire_xyzi()
    table.check(hist)
    assert IC.same_rows_as_set(hist, cloud[dead]) and IC.same_rows_as_set(reg.map_removed_acquire(), hist[:, :3])
    _assert_map_is(reg, cloud[~dead], table)
    # by point
    alive = cloud[~dead]
    pick = rng.choice(len(alive), 150, replace=False)
    assert reg.map_delete_points(alive[pick, :3]) == 150
    hist = reg.map_removed_acquire_xyzi(clear=True)
    assert IC.same_rows_as_set(hist, np.concatenate([cloud[dead], alive[pick]]))
    alive = np.delete(alive, pick, axis=0)
    _assert_map_is(reg, alive, table)
    assert len(reg.map_removed_acquire_xyzi()) == 0
    # by a move of the local-map cube: cube_len 40, det_range 5 - the cube starts as [-20, 20)^3 around the origin; at x = 15 the sensor is
    # within 1.5 x 5 of the +x face and the cube moves by 11.25: the slab x < -8.75 goes
    reg.local_map_set(40.0, 5.0, enabled=False)
    assert reg.local_map_segment([0.0, 0.0, 0.0])["n_deleted"] == 0
    info = reg.local_map_segment([15.0, 0.0, 0.0])
    slab = _in_boxes(alive, info["boxes"])
    assert info["n_boxes"] == 1 and info["n_deleted"] == int(slab.sum()) > 100
    hist = reg.map_removed_acquire_xyzi(clear=True)
    table.check(hist)
    assert IC.same_rows_as_set(hist, alive[slab])
    alive = alive[~slab]
    _assert_map_is(reg, alive, table)
    # overflow, as the sibling: the delete completes, what found room is intact, both forms report LII_ERR_CAPACITY
    reg.map_removed_set(10)
    box = np.array([[0, -19, -19, 19, 19, 19]], np.float32)
    gone = _in_boxes(alive, box)
    assert reg.map_delete_boxes(box) == int(gone.sum()) > 10
    assert _code(reg.map_removed_acquire_xyzi) == CAPACITY and _code(reg.map_removed_acquire) == CAPACITY
    held = reg.map_removed_acquire_xyzi(strict=False)
    assert len(held) == 10
    table.check(held)
    assert _in_boxes(held, box).all() and IC.same_rows_as_set(reg.map_removed_acquire(strict=False), held[:, :3])
    info = reg.map_removed_get()
    assert info["held"] == 10 and info["lost_total"] == int(gone.sum()) - 10
    _assert_map_is(reg, alive[~gone], table)
    # the view's records: the fourth float is the intensity
    L, h = reg.L, reg.h
    p, n = C.c_void_p(), C.c_int32(0)
    assert L.lii_map_removed_view(h, C.byref(p), C.byref(n)) == CAPACITY and n.value == 10
    rec = _dev_array(reg, p.value, (10, 4), "<f4")
    table.check(rec)
    # NULL arguments
    assert L.lii_map_removed_acquire_xyzi(h, None, 0, None, 0) == INVALID
    reg.close()


# ------------------------------------------------------------------------------------------------ queries
@pytest.fixture(scope="module")
def lived_in():
    """A map that has been through inserts (with and without down-sampling) and deletes: (registrar, table, live rows)."""
    rng = np.random.default_rng(75)
    cloud = IC.distinct_cloud(rng, 8300, lo=-6.0, hi=8.0)  # (one cloud, dealt out: distinct triples and intensities across the three parts)
    base, add, more = cloud[:6000], cloud[6000:7500], cloud[7500:]
    IC.assert_distinct_triples(base, add, more)
    table = IC.Table(base, add, more)
    reg = _registrar()
    reg.map_build_xyzi(base)
    reg.map_add_points_xyzi(add, True)
    reg.map_add_points_xyzi(IC.as_xyzinormal(more), False)
    reg.map_delete_boxes(np.array([[-1, -1, -6, 1, 1, 6]], np.float32))
    live = reg.map_download_xyzi()
    reg.map_delete_points(live[::7, :3])
    live = reg.map_download_xyzi()
    table.check(live)
    assert 4000 < len(live) < len(base) + len(add) + len(more)
    q = np.ascontiguousarray(np.r_[rng.uniform(-7, 10, (300, 3)), live[rng.choice(len(live), 40), :3], [[np.nan, 0, 0], [500.0, 0, 0]]].astype(np.float32))
    yield reg, table, live, q
    reg.close()


@pytest.mark.parametrize("k", (1, 5, 64))
def test_nearest_xyzi(lived_in, k):
    reg, table, live, q = lived_in
    md = 30.0 if k == 64 else 5.0
    p3, d3, c3 = reg.map_nearest(q, k=k, max_dist=md)
    p4, d4, c4 = reg.map_nearest_xyzi(q, k=k, max_dist=md)
    assert np.array_equal(c3, c4) and _same_bits(d3, d4) and _same_bits(p3, p4[..., :3])
    assert c4.max() == k and c4.min() == 0
    filled = np.arange(k)[None, :] < c4[:, None]
    table.check(p4[filled])
    assert (_bits(p4[~filled]) == 0).all()  # the rows from count[i] on are zeros, all four floats
    # the device form: stride-16 queries, the same rows
    n = len(q)
    wide = np.full((n, 4), 3.0, np.float32)
    wide[:, :3] = q
    d_q = _dev_filled(reg, wide)
    d_p, d_d, d_c = _dev_filled(reg, np.full((n, k, 4), -7.0, np.float32)), _dev_filled(reg, np.full((n, k), -7.0, np.float32)), _dev_filled(reg, np.full(n, -7, np.int32))
    reg.map_nearest_xyzi_dev(d_q, n, k, md, d_p, d_d, d_c, stride_bytes=16)
    assert np.array_equal(_dev_array(reg, d_c, (n,), "<i4"), c4) and _same_bits(_dev_array(reg, d_d, (n, k), "<f4"), d4)
    assert _same_bits(_dev_array(reg, d_p, (n, k, 4), "<f4"), p4)
    # one output left out
    assert reg.L.lii_map_nearest_xyzi(reg.h, q.ctypes.data, n, 12, k, C.c_double(md), None, None, c3.ctypes.data) == 0 and np.array_equal(c3, c4)


@pytest.mark.parametrize("sorted_", (False, True))
def test_radius_xyzi(lived_in, sorted_):
    reg, table, live, q = lived_in
    md = 1.0
    o3, p3, d3 = reg.map_radius(q, md, sorted=sorted_)
    o4, p4, d4 = reg.map_radius_xyzi(q, md, sorted=sorted_)
    assert np.array_equal(o3, o4) and _same_bits(d3, d4) and o4[-1] > 500
    if not sorted_:
        assert _same_bits(p3, p4[:, :3])
    else:  # (equal d2 inside a segment come in unspecified order: per query the same multiset of rows)
        for i in np.flatnonzero(np.diff(o4) > 0):
            assert IC.same_rows_as_set(p3[o3[i]:o3[i + 1]], p4[o4[i]:o4[i + 1], :3])
        assert all(np.all(np.diff(d4[o4[i]:o4[i + 1]]) >= 0) for i in range(len(q)))
    table.check(p4)
    # count only, and a capacity below the total: offsets and total written, nothing else
    assert np.array_equal(reg.map_radius_xyzi(q, md, sorted=sorted_, points=False)[0], o4)
    L, h = reg.L, reg.h
    total, n = int(o4[-1]), len(q)
    flags = 1 if sorted_ else 0
    oo, tt = np.full(n + 1, -7, np.int64), C.c_int64(-7)
    small_p, small_d = np.full((total - 1, 4), -7.0, np.float32), np.full(total - 1, -7.0, np.float32)
    assert L.lii_map_radius_xyzi(h, q.ctypes.data, n, 12, C.c_double(md), flags, oo.ctypes.data, small_p.ctypes.data, small_d.ctypes.data, total - 1, C.byref(tt)) == CAPACITY
    assert np.array_equal(oo, o4) and tt.value == total and (small_p == -7.0).all() and (small_d == -7.0).all()
    # the device form with a capacity below the total: the rows below it, the pattern above, the full total
    d_q = _dev_filled(reg, q)
    for cap in (total, total // 2):
        d_p, d_d = _dev_filled(reg, np.full((total, 4), -7.0, np.float32)), _dev_filled(reg, np.full(total, -7.0, np.float32))
        d_o, d_t = _dev_filled(reg, np.full(n + 1, -7, np.int64)), _dev_filled(reg, np.full(1, -7, np.int64))
        reg.map_radius_xyzi_dev(d_q, n, md, d_o, d_p, d_d, cap, d_t, sorted=sorted_)
        assert np.array_equal(_dev_array(reg, d_o, (n + 1,), "<i8"), o4) and _dev_array(reg, d_t, (1,), "<i8")[0] == total
        gp, gd = _dev_array(reg, d_p, (total, 4), "<f4"), _dev_array(reg, d_d, (total,), "<f4")
        assert (gp[cap:] == -7.0).all() and (gd[cap:] == -7.0).all()
        whole = cap if (cap == total or not sorted_) else int(o4[np.searchsorted(o4, cap, side="right") - 1])
        if not sorted_:
            assert _same_bits(gp[:whole], p4[:whole]) and _same_bits(gd[:whole], d4[:whole])
        else:
            assert _same_bits(gd[:whole], d4[:whole])
            for i in np.flatnonzero((np.diff(o4) > 0) & (o4[1:] <= whole)):
                assert IC.same_rows_as_set(gp[o4[i]:o4[i + 1]], p4[o4[i]:o4[i + 1]])
        table.check(gp[:cap])  # every row that was written is a stored point with its own intensity
    # count only on the device
    d_o, d_t = _dev_filled(reg, np.full(n + 1, -7, np.int64)), _dev_filled(reg, np.full(1, -7, np.int64))
    reg.map_radius_xyzi_dev(d_q, n, md, d_o, None, None, 0, d_t, sorted=sorted_)
    assert np.array_equal(_dev_array(reg, d_o, (n + 1,), "<i8"), o4)


def test_box_search_xyzi(lived_in):
    reg, table, live, q = lived_in
    boxes = np.array([[2, 2, -6, 5, 5, 6], [4, 4, -6, 8, 8, 6], [30, 30, 30, 40, 40, 40]], np.float32)
    inside = _in_boxes(live, boxes)
    assert (_in_boxes(live, boxes[:1]) & _in_boxes(live, boxes[1:2])).sum() > 5  # points in two boxes: once each
    got = reg.map_box_search_xyzi(boxes)
    table.check(got)
    assert IC.same_rows_as_set(got, live[inside]) and IC.same_rows_as_set(reg.map_box_search(boxes), got[:, :3])
    L, h = reg.L, reg.h
    n = C.c_int32(-1)
    assert L.lii_map_box_search_xyzi(h, boxes.ctypes.data, 3, None, 0, C.byref(n)) == 0 and n.value == int(inside.sum())
    small = np.full((n.value - 1, 4), 7.0, np.float32)
    assert L.lii_map_box_search_xyzi(h, boxes.ctypes.data, 3, small.ctypes.data, len(small), C.byref(n)) == CAPACITY and (small == 7.0).all()
    assert L.lii_map_box_search_xyzi(h, boxes.ctypes.data, 3, small.ctypes.data, len(small), None) == INVALID
    assert len(reg.map_box_search_xyzi(boxes[2:])) == 0


# ------------------------------------------------------------------------------------------------ the map as a PCD
def test_map_pcd(lived_in):
    import lidar_imu_init_amd as lii
    reg, table, live, q = lived_in
    rows = reg.map_pcd()
    assert rows.shape == (len(live), 32) and rows.dtype == np.uint8
    # a host repack of lii_map_download_xyzi, as a multiset
    want = np.zeros((len(live), 8), np.float32)
    want[:, :3] = live[:, :3]
    want[:, 6] = live[:, 3]
    assert IC.same_rows_as_set(np.ascontiguousarray(rows).view(np.float32).reshape(-1, 8), want)
    # header + rows parse back
    blob = lii.pcd_header(len(rows)) + rows.tobytes()
    head, _, data = blob.partition(b"DATA binary\n")
    fields = head.decode().split("FIELDS ")[1].split("\n")[0].split()
    assert fields == ["x", "y", "z", "normal_x", "normal_y", "normal_z", "intensity", "curvature"] and f"POINTS {len(rows)}\n" in head.decode()
    rec = np.frombuffer(data, np.dtype([(f, "<f4") for f in fields]))
    assert len(rec) == len(rows)
    back = np.c_[rec["x"], rec["y"], rec["z"], rec["intensity"]].astype(np.float32)
    table.check(back)
    assert IC.same_rows_as_set(back, live)
    assert all((rec[f].view(np.uint32) == 0).all() for f in ("normal_x", "normal_y", "normal_z", "curvature"))
    # count only, capacity refusal with nothing written, NULL
    L, h = reg.L, reg.h
    n = C.c_int32(-1)
    assert L.lii_map_pcd(h, None, 0, C.byref(n)) == 0 and n.value == len(live)
    small = np.full(32 * len(live) - 1, 7, np.uint8)
    assert L.lii_map_pcd(h, small.ctypes.data, C.c_int64(small.nbytes), C.byref(n)) == CAPACITY and n.value == len(live) and (small == 7).all()
    assert L.lii_map_pcd(h, small.ctypes.data, C.c_int64(small.nbytes), None) == INVALID
    # an observer: the map is as it was
    assert IC.same_rows_as_set(reg.map_download_xyzi(), live)


def test_map_pcd_crosses_a_staging_chunk(big_cloud):
    reg = _registrar()
    reg.map_build_xyzi(big_cloud)
    rows = np.ascontiguousarray(reg.map_pcd()).view(np.float32).reshape(-1, 8)
    assert len(rows) == len(big_cloud) > 65_536
    assert IC.same_rows_as_set(np.ascontiguousarray(rows[:, [0, 1, 2, 6]]), big_cloud) and (_bits(rows[:, [3, 4, 5, 7]]) == 0).all()
    reg.map_reset()
    assert reg.map_pcd().shape == (0, 32)
    reg.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_from_inside_while_waiting(small_world):
    import bench
    import lidar_imu_init_amd as lii
    from harness import synth
    hall, map_pts = small_world
    map_pts = np.unique(np.ascontiguousarray(map_pts, np.float32), axis=0)
    cloud = IC.with_intensity(map_pts)
    R, p = synth.rot_zyx(0.03, -0.02, 0.4), np.array([0.8, -0.6, 0.1])
    scan = synth.make_scan(hall, "vlp16", R, p, noise=0.02, seed=31)
    scan = scan[np.argsort(scan[:, 3], kind="stable")]
    st = lii.State()
    st.rot_end[:] = R
    st.pos_end[:] = p
    prop = st.copy()
    reg = lii.Registrar(max_scan_points=40_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build_xyzi(cloud)
    L, h = reg.L, reg.h
    q = np.ascontiguousarray(map_pts[:16])
    d_q = _dev_filled(reg, q)
    d_o, d_t = _dev_filled(reg, np.full(17, -7, np.int64)), _dev_filled(reg, np.full(1, -7, np.int64))
    seen = []

    def hook():
        n, tt, oo = C.c_int32(-7), C.c_int64(-7), np.full(17, -7, np.int64)
        seen.append(L.lii_map_pcd(h, None, 0, C.byref(n)))
        seen.append(L.lii_map_radius_xyzi(h, q.ctypes.data, 16, 12, C.c_double(1.0), 0, oo.ctypes.data, None, None, 0, C.byref(tt)))
        seen.append(L.lii_map_radius_xyzi_dev(h, d_q, 16, 12, C.c_double(1.0), 0, d_o, None, None, 0, d_t))
        seen.append(L.lii_map_removed_acquire_xyzi(h, None, 0, C.byref(n), 0))
        seen.append(int(n.value == -7 and tt.value == -7 and (oo == -7).all()))

    reg.scan_register(st, prop, imu_poses=bench.pose_table(prop.rot_end, prop.pos_end), leaf=0.1, max_iterations=5, imu_en=True, scan_dev=reg.device_scan(scan),
                      scan_sorted=True, while_waiting=hook)
    assert seen == [STATE, STATE, STATE, STATE, 1]
    # ... and the registration ran against a map with intensities as against any other: the map still holds them
    IC.Table(cloud).check(reg.map_download_xyzi())
    reg.close()


# ------------------------------------------------------------------------------------------------ scan-driven updates: lii_map_intensity_set
def _world_of(body, st):
    """pointBodyToWorld as the decision kernel forms it: doubles, products added left to right, the result stored to float (the world
    point whose bits the map keeps); st: a lii.State."""
    b = np.ascontiguousarray(body, np.float32)[:, :3].astype(np.float64)
    RLI, TLI, R, p = (np.asarray(a, np.float64) for a in (st.offset_R_L_I, st.offset_T_L_I, st.rot_end, st.pos_end))
    i = [(RLI[r, 0] * b[:, 0] + RLI[r, 1] * b[:, 1]) + RLI[r, 2] * b[:, 2] + TLI[r] for r in range(3)]
    w = [(R[r, 0] * i[0] + R[r, 1] * i[1]) + R[r, 2] * i[2] + p[r] for r in range(3)]
    return np.ascontiguousarray(np.stack(w, axis=1).astype(np.float32))


def _scan_table(reg, st):
    """xyz bits of every down-sampled point's world point -> the intensity lii_scan_intensity_download(h, 1) returns for it (held to the
    oracle by tests/test_gpu_intensity.py), joined by index with lii_scan_download(h, 1); None when no intensities are attached."""
    body = reg.scan_download(1)
    world = _world_of(body, st)
    try:
        inten = reg.scan_intensity_download(1)
    except Exception:
        return world, None
    assert len(inten) == len(world)
    return world, np.ascontiguousarray(np.c_[world, inten], np.float32)


def _voxel_winners(cloud, ds):
    """Per down-sample voxel of a cloud that meets no stored point: the point closest to the voxel's centre (what Add_Points keeps)."""
    vox, d2 = IC.voxel_of(cloud, ds), IC.centre_d2(cloud, ds)
    keep = np.zeros(len(cloud), bool)
    order = np.lexsort((d2, vox[:, 2], vox[:, 1], vox[:, 0]))
    first = np.r_[True, (np.diff(vox[order], axis=0) != 0).any(axis=1)]
    keep[order[first]] = True
    return cloud[keep]


def _identity_state(oracle):
    import lidar_imu_init_amd as lii
    st = lii.State(oracle.state_init())
    assert np.array_equal(st.rot_end, np.eye(3)) and not st.pos_end.any() and np.array_equal(st.offset_R_L_I, np.eye(3)) and not st.offset_T_L_I.any()
    return st


def _incremental_world(seed):
    """A small map with intensities, a scan registered against it (map points + noise: neighbour lists, both insert lists) and a scan far from
    it (no neighbour inside max_match_dist: every point added), all with distinct triples and intensities."""
    rng = np.random.default_rng(seed)
    base = IC.distinct_cloud(rng, 3000, lo=-5.0, hi=5.0)
    near = (base[rng.choice(len(base), 1500), :3] + rng.normal(0, 0.15, (1500, 3))).astype(np.float32)
    near = IC.with_intensity(np.unique(near, axis=0), first=10_000)
    far = IC.distinct_cloud(rng, 900, lo=60.0, hi=70.0, first=20_000)
    IC.assert_distinct_triples(base, near, far)
    far2 = IC.distinct_cloud(rng, 5, lo=80.0, hi=90.0, first=30_000)  # (five points: the smallest launch)
    return base, near[rng.permutation(len(near))], far, far2


@pytest.mark.parametrize("mode", ("counts", "no_counts", "fold_sort", "map_tight"))
def test_map_incremental_with_the_switch_on(oracle, mode):
    """lii_map_incremental with the switch on and intensities attached: the hashed fold (its leader keeps p0.w), the second list, the same
    with predicted list sizes (want_counts=False), under LII_TEST=fold_sort (the sorted fold) and map_tight (parked inserts).  The identity
    state makes the world point the body point bit for bit: the surviving triples are the oracle's map_incremental + flatten, the
    intensity of each is a lookup by its triple."""
    base, near, far, far2 = _incremental_world(80)
    ds = IC.DS
    reg = _registrar(env=mode if mode in ("fold_sort", "map_tight") else None)
    assert reg.map_intensity_get() is False
    reg.map_intensity_set(True)
    assert reg.map_intensity_get() is True
    reg.map_build_xyzi(base)
    tree = oracle.Tree("oracle", downsample=ds)
    tree.build(base[:, :3])
    table = IC.Table(base)
    st = _identity_state(oracle)
    for scan in (near, far, far2):
        reg.scan_upload(np.c_[scan[:, :3], np.zeros(len(scan), np.float32)])
        reg.scan_intensity_upload(np.ascontiguousarray(scan[:, 3]))
        n = reg.downsample_skip()
        reg.iekf_iterate(st, True, False)
        world, rows = _scan_table(reg, st)
        assert rows is not None and IC.same_rows_as_set(rows, scan)  # identity state: the world point is the input point, with its intensity
        table.add(rows)
        body4 = reg.scan_download(1)
        # the oracle's lists: its neighbour lists come from the search of an update's first iteration - at the identity state, where the
        # device searched - and its decision is made at the identity state as well (test_gpu_map.py obtains them the same way)
        tree.iekf_update(body4, st.pod.copy(), st.pod.copy(), max_iterations=1, imu_en=False, threads=4)
        a, b = tree.map_incremental(body4, st.pod, ds, apply=True)
        got = reg.map_incremental(st, want_counts=(mode != "no_counts"))
        if got is not None:
            assert got == (len(a), len(b))
        if scan is far:
            assert len(a) == len(far) and len(b) == 0  # no neighbour lists: every point goes into the down-sampled list
        elif scan is near:
            assert len(a) > 100 and len(b) > 20  # both lists
    live = reg.map_download_xyzi()
    table.check(live)
    assert IC.same_rows_as_set(live[:, :3], tree.flatten())
    assert (live[:, 3] != 0).all()
    # the scans far from the map met no stored point: what they left is the closest-to-centre point of each of their voxels, with its intensity
    for cloud, lo in ((far, 55.0), (far2, 75.0)):
        mine = live[(live[:, 0] >= lo) & (live[:, 0] < lo + 20.0)]
        assert IC.same_rows_as_set(mine, _voxel_winners(cloud, ds))
    assert np.isin(_bits(live[:, 3]), _bits(near[:, 3])).sum() > 100
    # the world points of the last iteration keep their fourth float 0
    assert (_bits(reg.scan_download(2)[:, 3]) == 0).all()
    tree.close()
    reg.close()


def test_switch_on_without_intensities_and_switch_off_store_zeros(oracle):
    base, near, far, _ = _incremental_world(81)
    st = _identity_state(oracle)
    for on, attach in ((True, False), (False, True), (False, False)):
        reg = _registrar()
        if on:
            reg.map_intensity_set(True)
        reg.map_build_xyzi(base)
        reg.scan_upload(np.c_[near[:, :3], np.zeros(len(near), np.float32)])
        if attach:
            reg.scan_intensity_upload(np.ascontiguousarray(near[:, 3]))
        reg.downsample_skip()
        reg.iekf_iterate(st, True, False)
        na, nn = reg.map_incremental(st)
        assert na > 100 and nn > 20
        live = reg.map_download_xyzi()
        old = np.isin(_bits(live[:, 3]), _bits(base[:, 3]))  # (the map's own intensities are never zero)
        IC.Table(base).check(live[old])
        assert (~old).sum() > 100 and (_bits(live[~old, 3]) == 0).all(), (on, attach)
        reg.close()


def _job_world(small_world):
    import lidar_imu_init_amd as lii
    from harness import synth
    hall, map_pts = small_world
    cloud = IC.with_intensity(np.unique(np.ascontiguousarray(map_pts, np.float32), axis=0))
    R, p = synth.rot_zyx(0.03, -0.02, 0.4), np.array([0.8, -0.6, 0.1])
    scan = synth.make_scan(hall, "vlp16", R, p, noise=0.02, seed=31)
    scan = np.ascontiguousarray(scan[np.argsort(scan[:, 3], kind="stable")], np.float32)
    st = lii.State()
    st.rot_end[:] = R
    st.pos_end[:] = p
    inten = (np.arange(len(scan), dtype=np.float64) * 0.5 + 100_000.0).astype(np.float32)  # (above every map intensity: told apart by value)
    assert inten.min() > cloud[:, 3].max()
    return cloud, scan, inten, st


def _launches(reg):
    return {k: v[1] for k, v in reg.kernel_profile()[0].items()}


def test_map_update_inside_the_job(small_world):
    """lii_scan_job::map_update with the switch on: every point the update inserts carries the intensity of its down-sampled point (PCL's
    centroid of the voxel's members, lii_scan_intensity_download(h, 1)), looked up by the bits of its world point at the final state.  The
    switch adds no launch: lii_set_profiling(h, 3) counts the same per kind with it off, on, and on a handle that never saw it - and off
    stores zeros."""
    import bench
    import lidar_imu_init_amd as lii
    cloud, scan, inten, st0 = _job_world(small_world)
    counts, news = {}, {}
    for form in ("never", "on", "off_again"):
        reg = lii.Registrar(max_scan_points=40_000, max_map_points=400_000, filter_size_map=0.15)
        if form != "never":
            reg.map_intensity_set(True)
        if form == "off_again":
            reg.map_intensity_set(False)
        reg.map_build_xyzi(cloud)
        n0 = reg.map_size()
        reg.set_profiling(1)
        reg.set_profiling(3)
        reg.scan_upload(scan)
        reg.scan_intensity_upload(inten)
        st, prop = st0.copy(), st0.copy()
        rep = reg.scan_register(st, prop, imu_poses=bench.pose_table(prop.rot_end, prop.pos_end), leaf=0.1, max_iterations=5, imu_en=True,
                                scan_sorted=True, map_update=True)
        assert rep["effect_num"] > 500
        counts[form] = _launches(reg)
        live = reg.map_download_xyzi()
        assert len(live) == reg.map_size() > n0 - 50
        zero, big = _bits(live[:, 3]) == 0, live[:, 3] >= 100_000.0  # (map intensities are k + 0.25 < 100 000: never zero; the scan's lie above)
        IC.Table(cloud).check(live[~zero & ~big])
        if form == "on":
            world, rows = _scan_table(reg, st)
            assert rows is not None and zero.sum() == 0 and big.sum() > 100
            IC.assert_distinct_triples(rows)
            IC.Table(rows).check(live[big])   # (KeyError: a stored triple that is no world point of the down-sampled cloud)
        else:
            assert big.sum() == 0 and zero.sum() > 100
        news[form] = int((zero | big).sum())
        print(form, counts[form], news[form])
        reg.close()
    assert counts["never"] == counts["on"] == counts["off_again"]
    assert news["never"] == news["on"] == news["off_again"]  # the same points are inserted, with and without their intensities


def test_build_from_scan_with_the_switch_on(oracle):
    rng = np.random.default_rng(82)
    scan = IC.distinct_cloud(rng, 700, lo=-8.0, hi=8.0)
    st = _identity_state(oracle)
    for on in (True, False):
        reg = _registrar()
        reg.map_intensity_set(on)
        reg.scan_upload(np.c_[scan[:, :3], np.zeros(len(scan), np.float32)])
        reg.scan_intensity_upload(np.ascontiguousarray(scan[:, 3]))
        reg.downsample_skip()
        assert reg.map_build_from_scan(st) == len(scan)
        live = reg.map_download_xyzi()
        if on:
            IC.Table(scan).check(live)
            assert IC.same_rows_as_set(live, scan)
            assert IC.same_rows_as_set(np.ascontiguousarray(reg.map_pcd()).view(np.float32).reshape(-1, 8)[:, [0, 1, 2, 6]], scan)
        else:
            assert IC.same_rows_as_set(live[:, :3], scan[:, :3]) and (_bits(live[:, 3]) == 0).all()
        reg.close()


def test_switch_refusals(small_world):
    import bench
    import lidar_imu_init_amd as lii
    # with a communicator attached; and lii_comm_init on a handle with the switch on
    reg = _registrar()
    reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")
    assert _code(reg.map_intensity_set, True) == STATE and _code(reg.map_intensity_set, False) == STATE
    assert reg.map_intensity_get() is False
    reg.close()
    reg = _registrar()
    reg.map_intensity_set(True)
    assert _code(reg.comm_init, 1, 0, reg.comm_unique_id(), "rccl") == STATE
    assert reg.map_intensity_get() is True and reg.comm_describe() == "no communicator"
    L, h = reg.L, reg.h
    assert L.lii_map_intensity_set(h, 2) == INVALID and L.lii_map_intensity_set(h, -1) == INVALID and L.lii_map_intensity_get(h, None) == INVALID
    assert reg.map_intensity_get() is True
    reg.map_intensity_set(False)
    reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")  # off: a communicator attaches as ever
    reg.close()
    # from inside lii_scan_job::while_waiting
    cloud, scan, inten, st = _job_world(small_world)
    reg = lii.Registrar(max_scan_points=40_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build_xyzi(cloud)
    L, h = reg.L, reg.h
    seen = []

    def hook():
        on = C.c_int32(-7)
        seen.append(L.lii_map_intensity_set(h, 1))
        seen.append(L.lii_map_intensity_get(h, C.byref(on)))
        seen.append(on.value)

    prop = st.copy()
    reg.scan_register(st, prop, imu_poses=bench.pose_table(prop.rot_end, prop.pos_end), leaf=0.1, max_iterations=5, imu_en=True, scan_dev=reg.device_scan(scan),
                      scan_sorted=True, while_waiting=hook)
    assert seen == [STATE, STATE, -7] and reg.map_intensity_get() is False
    reg.close()


def test_switch_under_host_solve(oracle):
    """LII_TEST=host_solve: the switch can be set; no intensities can be attached there, so the update stores zeros."""
    base, near, far, _ = _incremental_world(83)
    reg = _registrar(env="host_solve")
    reg.map_intensity_set(True)
    reg.map_build_xyzi(base)
    st = _identity_state(oracle)
    reg.scan_upload(np.c_[far[:, :3], np.zeros(len(far), np.float32)])
    assert _code(reg.scan_intensity_upload, np.ascontiguousarray(far[:, 3])) == STATE
    reg.downsample_skip()
    reg.iekf_iterate(st, True, False)
    assert reg.map_incremental(st) == (len(far), 0)
    live = reg.map_download_xyzi()
    old = live[:, 0] < 50
    IC.Table(base).check(live[old])
    assert IC.same_rows_as_set(live[~old, :3], _voxel_winners(far, IC.DS)[:, :3]) and (_bits(live[~old, 3]) == 0).all()
    reg.close()
