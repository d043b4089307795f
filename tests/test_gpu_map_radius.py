"""lii_map_radius / lii_map_radius_dev: the ball query - every map point within max_dist of a point, however many there are.

Expected values: the float32 brute-force balls of tests/map_radius_cases.py (calc_dist's evaluation order), and for max_dist >= 1 the
UNMODIFIED reference tree's large-k Nearest_Search where oracle/_ref is built - never the library.  Every comparison is exact: offsets
equal, per query the multiset of d2 bits equal, per query the multiset of point rows equal (tests/test_map_radius_ref.py shows on the
CPU that the reference tree meets the same brute force)."""
import ctypes as C

import numpy as np
import pytest

from map_nearest_cases import d2_f32
from map_radius_cases import FAR_EVERY_GPU, Balls, check_radius, check_same_balls, rows_at_their_d2, small_world_balls, tree_balls

pytestmark = pytest.mark.gpu

INVALID, STATE, CAPACITY = -1, -5, -4
SORTED = 1


@pytest.fixture(scope="module")
def world_reg(small_world):
    import lidar_imu_init_amd as lii
    map_pts = np.ascontiguousarray(small_world[1], np.float32)
    reg = lii.Registrar(max_scan_points=10_000, max_map_points=100_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    yield reg
    reg.close()


@pytest.fixture(scope="module")
def world_ref(oracle, small_world):
    if not oracle.ref_available():
        return None
    tree = oracle.Tree("ref")
    tree.build(np.ascontiguousarray(small_world[1], np.float32))
    return tree


def _dev_array(reg, addr, shape, typestr):
    """device memory -> numpy, through the runtime the library itself uses (symbols looked up through its own handle)"""
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


# ------------------------------------------------------------------------------------------------ 1. parity on small_world
@pytest.mark.parametrize("max_dist", (0.0, 0.04, 0.81, 1.0, 5.0, 30.0))
def test_parity_with_brute_force_and_reference_tree(world_reg, world_ref, small_world, max_dist):
    """0.81 = (2 x 0.45)^2: the radius is a whole number of cells; 5 crosses the 2^20-row chunk, 30 (every 4th query) several times."""
    q, balls = small_world_balls(small_world)
    sel = np.arange(0, len(q), FAR_EVERY_GPU if max_dist > 5.0 else 1)
    qs = np.ascontiguousarray(q[sel])
    expected = balls.case(max_dist, sel)
    off, pts, d2 = world_reg.map_radius(qs, max_dist)
    check_radius(off, pts, d2, expected, balls.pts, f"lii_map_radius max_dist={max_dist}", q=qs)
    if max_dist >= 5.0:
        assert off[-1] > 1 << 20  # more than one chunk of rows
    if max_dist <= 5.0:
        assert off[-1] == off[-2] == off[-3]  # the query at 1e7 m and the NaN query: empty segments
    if max_dist == 0.0:
        assert off[-1] >= 500 and not d2.any()  # the queries that ARE map points find themselves
    if world_ref is not None and max_dist >= 1.0:
        k = int(np.diff(expected[0]).max()) + 1
        check_same_balls(off, pts, d2, tree_balls(world_ref, qs, max_dist, k), f"lii_map_radius against the reference tree, k = {k}, max_dist = {max_dist}")


# ------------------------------------------------------------------------------------------------ 2. batch edges in a crowded cell
def test_batch_edges_in_a_crowded_cell_and_the_inclusive_bound():
    """Balls of exactly 0, 1, 63, 64, 65, 128, 129 and 5 000 points, each inside one grid cell of a hand-made map; a point at d2 ==
    max_dist exactly is in, at the next double below it is out."""
    import lidar_imu_init_amd as lii
    rng = np.random.default_rng(11)
    cs = 0.45
    pops = (0, 1, 63, 64, 65, 128, 129, 5000)
    centres = np.array([[(8 * i + 4.5) * cs, 20.5 * cs, -7.5 * cs] for i in range(len(pops))])  # cell centres, 8 cells apart
    clouds = [(c + rng.uniform(-0.1, 0.1, (p, 3))).astype(np.float32) for c, p in zip(centres, pops)]  # all within sqrt(0.03) < 0.2 m
    pts = np.concatenate(clouds + [np.array([[1, 0, 0]], np.float32), rng.uniform(-12, -2, (2000, 3)).astype(np.float32)])
    reg = lii.Registrar(max_scan_points=5000, max_map_points=20_000, filter_size_map=0.15)
    reg.map_build(pts)
    assert reg.map_size() == len(pts)
    q = centres.astype(np.float32)
    for flag in (False, True):
        off, p, d = reg.map_radius(q, 0.04, sorted=flag)
        assert np.diff(off).tolist() == list(pops)
        check_radius(off, p, d, Balls(q, pts, 0.04).case(0.04), pts, f"crowded cells, sorted={flag}", q=q)
        if flag:
            assert all(np.all(np.diff(d[a:b]) >= 0) for a, b in zip(off[:-1], off[1:]))
    # wider balls over the same map (the crowded cells among their neighbours)
    for md in (1.0, 3.0):
        off, p, d = reg.map_radius(q, md)
        check_radius(off, p, d, Balls(q, pts, md).case(md), pts, f"crowded cells, max_dist={md}", q=q)
    origin = np.zeros((1, 3), np.float32)
    assert d2_f32(origin, pts)[0].min() == 1.0  # (1, 0, 0) is the nearest point, at d2 == 1 exactly
    off, p, d = reg.map_radius(origin, 1.0)
    assert off.tolist() == [0, 1] and p.tolist() == [[1.0, 0.0, 0.0]] and d.tolist() == [1.0]
    off, p, d = reg.map_radius(origin, float(np.nextafter(1.0, 0.0)))
    assert off.tolist() == [0, 0] and len(p) == 0 and len(d) == 0
    reg.close()


# ------------------------------------------------------------------------------------------------ 3. the ring bound
def test_the_ring_bound_is_exact(world_reg, small_world):
    q, balls = small_world_balls(small_world)
    cell = np.float32(3.0) * np.float32(0.15)  # map_cell_size as the handle derives it from filter_size_map
    edge = (32.0 * float(cell)) ** 2  # exact in a double: the square of a 24-bit number
    assert abs(edge - 207.36) < 1e-3 and np.sqrt(edge) == 32.0 * float(cell)
    two = np.ascontiguousarray(q[[600, 1100]])  # one near a surface, one inside the hall
    off, p, d = world_reg.map_radius(two, edge)
    check_radius(off, p, d, Balls(two, balls.pts, edge).case(edge), balls.pts, "the largest ball", q=two)
    assert off[-1] > len(balls.pts)  # two balls of radius 14.4 m: most of the hall each
    with pytest.raises(Exception) as e:
        world_reg.map_radius(two, float(np.nextafter(edge, np.inf)))
    assert e.value.code == INVALID and b"0.450" in world_reg.L.lii_last_error(world_reg.h)


# ------------------------------------------------------------------------------------------------ 4. LII_RADIUS_SORTED
@pytest.mark.parametrize("max_dist", (0.04, 5.0))
def test_sorted_segments_ascend_and_the_order_is_deterministic(world_reg, small_world, max_dist):
    q, balls = small_world_balls(small_world)
    off, p, d = world_reg.map_radius(q, max_dist)
    off2, p2, d2 = world_reg.map_radius(q, max_dist)
    assert np.array_equal(off, off2) and np.array_equal(p.view(np.uint32), p2.view(np.uint32)) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))
    so, sp, sd = world_reg.map_radius(q, max_dist, sorted=True)
    assert np.array_equal(so, off)
    inner = np.ones(len(sd), bool)
    inner[off[:-1][off[:-1] < len(sd)]] = False  # the first row of every segment has no predecessor in it
    assert np.all((np.diff(sd, prepend=np.float32(0)) >= 0) | ~inner)
    check_same_balls(so, sp, sd, (off, p, d), f"sorted against unsorted, max_dist={max_dist}")
    assert rows_at_their_d2(q, so, sp, sd)
    check_radius(so, sp, sd, balls.case(max_dist), balls.pts, f"sorted, max_dist={max_dist}")


# ------------------------------------------------------------------------------------------------ 5. count-only, capacity, strides
def test_count_only_capacity_and_strides(world_reg, small_world):
    q, balls = small_world_balls(small_world)
    L, h, n = world_reg.L, world_reg.h, len(q)
    off, p, d = world_reg.map_radius(q, 1.0)
    total = int(off[-1])
    o2, p2, d2 = world_reg.map_radius(q, 1.0, points=False)
    assert np.array_equal(o2, off) and len(p2) == 0 and len(d2) == 0
    # count-only through the C-ABI: capacity is ignored
    o3, t3 = np.full(n + 1, -7, np.int64), C.c_int64(-7)
    assert L.lii_map_radius(h, q.ctypes.data, n, 12, 1.0, 0, o3.ctypes.data, None, None, -5, C.byref(t3)) == 0
    assert np.array_equal(o3, off) and t3.value == total
    # capacity one row short: offsets and total written, the outputs untouched
    sent_p, sent_d = np.full((total, 3), -7.0, np.float32), np.full(total, -7.0, np.float32)
    for flags in (0, SORTED):
        pp, dd, o4, t4 = sent_p.copy(), sent_d.copy(), np.full(n + 1, -7, np.int64), C.c_int64(-7)
        assert L.lii_map_radius(h, q.ctypes.data, n, 12, 1.0, flags, o4.ctypes.data, pp.ctypes.data, dd.ctypes.data, total - 1, C.byref(t4)) == CAPACITY
        assert np.array_equal(o4, off) and t4.value == total and np.array_equal(pp, sent_p) and np.array_equal(dd, sent_d)
    # one output only
    dd, o5, t5 = sent_d.copy(), np.zeros(n + 1, np.int64), C.c_int64(0)
    assert L.lii_map_radius(h, q.ctypes.data, n, 12, 1.0, 0, o5.ctypes.data, None, dd.ctypes.data, total, C.byref(t5)) == 0
    assert np.array_equal(o5, off) and np.array_equal(dd.view(np.uint32), d.view(np.uint32))
    pp = sent_p.copy()
    assert L.lii_map_radius(h, q.ctypes.data, n, 12, 1.0, 0, o5.ctypes.data, pp.ctypes.data, None, total + 10, C.byref(t5)) == 0
    assert np.array_equal(pp.view(np.uint32), p.view(np.uint32))
    for width in (4, 12):  # strides 16 and 48
        wide = np.full((n, width), 7.0, np.float32)
        wide[:, :3] = q
        ow, pw, dw = world_reg.map_radius(wide, 1.0)
        assert wide.strides[0] == 4 * width and np.array_equal(ow, off) and np.array_equal(pw.view(np.uint32), p.view(np.uint32)) and np.array_equal(dw.view(np.uint32), d.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 6. more queries than one chunk
def test_seventy_thousand_queries(world_reg, small_world):
    q, balls = small_world_balls(small_world)
    off, p, d = world_reg.map_radius(q, 0.04)
    check_radius(off, p, d, balls.case(0.04), balls.pts, "one chunk of queries", q=q)
    rep = np.tile(q, (35, 1))  # 70 000 queries: two chunks of queries
    ob, pb, db = world_reg.map_radius(rep, 0.04)
    cnt = np.tile(np.diff(off), 35)
    assert np.array_equal(ob, np.concatenate([[0], np.cumsum(cnt)]))
    assert np.array_equal(pb.view(np.uint32), np.tile(p, (35, 1)).view(np.uint32)) and np.array_equal(db.view(np.uint32), np.tile(d, 35).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 7. a map that has changed
def _check_against_download(reg, q, what):
    """the query answers from the map AS IT IS: brute force over the downloaded map"""
    res = {md: reg.map_radius(q, md) for md in (0.09, 1.0, 5.0)}
    now = reg.map_download()
    balls = Balls(q, now, 5.0)
    for md, (off, p, d) in res.items():
        check_radius(off, p, d, balls.case(md), now, f"{what}, max_dist={md}", q=q)
    return now


def test_a_map_that_has_changed():
    """Behind lii_map_delete_boxes, lii_map_delete_points and lii_map_add_points (down-sampled and not) the balls come from the map as it is."""
    import lidar_imu_init_amd as lii
    rng = np.random.default_rng(21)
    ds = 0.3
    base = np.c_[rng.uniform(-10, 10, (20_000, 2)), rng.normal(0, 0.03, 20_000)].astype(np.float32)
    reg = lii.Registrar(max_scan_points=30_000, max_map_points=100_000, filter_size_map=ds)
    reg.map_build(base)
    q = np.concatenate([(base[rng.choice(len(base), 300)] + rng.normal(0, 0.1, (300, 3))), rng.uniform(-14, 14, (100, 3)) * [1, 1, 0.2]]).astype(np.float32)
    _check_against_download(reg, q, "built")
    add = (base[rng.choice(len(base), 3000)] + rng.normal(0, 0.2, (3000, 3))).astype(np.float32)
    reg.map_add_points(add, True)
    _check_against_download(reg, q, "after add_points(down-sampled)")
    plain = np.concatenate([rng.uniform([10.5, -3, -0.2], [13, 3, 0.2], (1500, 3)), rng.normal([1.0, 2.0, 0.3], 0.05, (500, 3))]).astype(np.float32)
    reg.map_add_points(plain, False)
    now = _check_against_download(reg, q, "after add_points(plain)")
    assert len(now) == reg.map_size()
    boxes = np.array([[-2, -2, -2, 2, 2, 2], [10, -10, -1, 14, 0, 1]], np.float32)
    assert reg.map_delete_boxes(boxes) > 1000
    now = _check_against_download(reg, q, "after delete_boxes")
    gone = np.ascontiguousarray(now[rng.choice(len(now), 2000, replace=False)])
    n_del = C.c_int32(0)
    reg._check(reg.L.lii_map_delete_points(reg.h, gone.ctypes.data, len(gone), 12, C.byref(n_del)))
    assert n_del.value == 2000
    now = _check_against_download(reg, q, "after delete_points")
    assert len(now) == reg.map_size()
    reg.close()


# ------------------------------------------------------------------------------------------------ 8. a map update in flight / 10. observer
def _scan_stream(hall, k):
    from harness import synth
    from harness.lo_harness import so3_exp
    import lidar_imu_init_amd as lii
    R = synth.rot_zyx(0.03, -0.02, 0.4 + 0.05 * k)
    p = np.array([0.8 + 0.1 * k, -0.6, 0.1])
    scan = synth.make_scan(hall, "vlp16", R, p, noise=0.02, seed=31 + k)
    scan = scan[np.argsort(scan[:, 3], kind="stable")]
    st = lii.State()
    st.rot_end[:] = R @ so3_exp(np.array([0.003, -0.002, 0.004]))
    st.pos_end[:] = p + np.array([0.03, -0.02, 0.01])
    return scan, st


def test_query_while_the_map_update_of_a_registration_is_under_way(small_world):
    """lii_scan_job::map_update leaves the in-place update running behind the call; a ball query made right away joins it first."""
    import bench
    import lidar_imu_init_amd as lii
    hall, map_pts = small_world
    q = np.ascontiguousarray(small_world_balls(small_world)[0][::8])
    reg = lii.Registrar(max_scan_points=40_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    n0 = reg.map_size()
    for k in range(2):
        scan, st = _scan_stream(hall, k)
        prop = st.copy()
        table = bench.pose_table(prop.rot_end, prop.pos_end)
        reg.scan_register(st, prop, imu_poses=table, leaf=0.1, max_iterations=5, imu_en=True, scan_dev=reg.device_scan(scan), scan_sorted=True, map_update=True)
        off, p, d = reg.map_radius(q, 1.0)  # (the update is still under way)
        now = reg.map_download()
        check_radius(off, p, d, Balls(q, now, 1.0).case(1.0), now, f"behind scan {k} with map_update", q=q)
    assert len(now) > n0  # the updates did add points
    reg.close()


def _run_stream(small_world, with_queries):
    import bench
    import lidar_imu_init_amd as lii
    hall, map_pts = small_world
    q = small_world_balls(small_world)[0]
    reg = lii.Registrar(max_scan_points=40_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    d_q = _dev_filled(reg, np.ascontiguousarray(q[:200]))
    d_o, d_p, d_d, d_t = reg.dev_alloc(201 * 8), reg.dev_alloc(100_000 * 12), reg.dev_alloc(100_000 * 4), reg.dev_alloc(8)
    states, reports, nbrs = [], [], []
    for k in range(3):
        scan, st = _scan_stream(hall, k)
        prop = st.copy()
        table = bench.pose_table(prop.rot_end, prop.pos_end)
        if with_queries:
            reg.map_radius(q[:300], 1.0)
        rep = reg.scan_register(st, prop, imu_poses=table, leaf=0.1, max_iterations=5, imu_en=True, scan_dev=reg.device_scan(scan), scan_sorted=True,
                                map_update=(k == 1))
        if with_queries:
            reg.map_radius(q[::5], 5.0, sorted=True)  # (scan 1: its map update is still under way)
        nd = len(reg.scan_download(1))
        nbrs.append(reg.neighbors(nd))
        if k != 1:
            reg.map_incremental(st, want_counts=(k == 0))
            if with_queries:
                reg.map_radius_dev(d_q, 200, 1.0, d_o, d_p, d_d, 100_000, d_t)  # (scan 2: the update runs beside it on its own stream)
        states.append(st.pod.copy())
        reports.append([rep["iterations"], rep["searches"], rep["effect_num"], int(rep["converged"])] + list(rep["normal_eq"]))
    final = reg.map_download()
    reg.close()
    return np.array(states), np.array(reports), nbrs, final[np.lexsort(final.T)]


def test_queries_do_not_disturb_a_registration_stream(small_world):
    """Two handles run the same 3-scan stream; one is queried between the scans.  States, reports, neighbour lists and map sets are equal."""
    a = _run_stream(small_world, False)
    b = _run_stream(small_world, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    for (pa, ca, sa), (pb, cb, sb) in zip(a[2], b[2]):
        assert np.array_equal(ca, cb) and np.array_equal(sa, sb) and np.array_equal(pa, pb)


# ------------------------------------------------------------------------------------------------ 9. device form
@pytest.mark.parametrize("flag", (False, True))
def test_device_form_equals_host_form(world_reg, small_world, flag):
    q, _ = small_world_balls(small_world)
    reg, n = world_reg, len(q)
    wide = np.full((n, 4), 3.0, np.float32)  # stride 16: a float4 cloud
    wide[:, :3] = q
    d_q = _dev_filled(reg, wide)
    for md in (0.04, 1.0):
        ho, hp, hd = reg.map_radius(q, md, sorted=flag)
        total = int(ho[-1])
        for cap in (total, total // 2):  # exact, and too small: the rows below capacity, the pattern above, the full total
            sent_p, sent_d = np.full((total, 3), -7.0, np.float32), np.full(total, -7.0, np.float32)
            d_p, d_d = _dev_filled(reg, sent_p), _dev_filled(reg, sent_d)
            d_o, d_t = _dev_filled(reg, np.full(n + 1, -7, np.int64)), _dev_filled(reg, np.full(1, -7, np.int64))
            reg.map_radius_dev(d_q, n, md, d_o, d_p, d_d, cap, d_t, sorted=flag, stride_bytes=16)
            reg.synchronize()
            assert np.array_equal(_dev_array(reg, d_o, (n + 1,), "<i8"), ho) and _dev_array(reg, d_t, (1,), "<i8")[0] == total
            gp, gd = _dev_array(reg, d_p, (total, 3), "<f4"), _dev_array(reg, d_d, (total,), "<f4")
            assert np.array_equal(gp[cap:], sent_p[cap:]) and np.array_equal(gd[cap:], sent_d[cap:])
            if cap == total or not flag:
                assert np.array_equal(gd[:cap].view(np.uint32), hd[:cap].view(np.uint32)) and np.array_equal(gp[:cap].view(np.uint32), hp[:cap].view(np.uint32))
            else:
                # sorted with too few rows: the segments below capacity are whole and equal; the cut one holds rows of its own ball
                whole = int(ho[np.searchsorted(ho, cap, side="right") - 1])
                assert np.array_equal(gd[:whole].view(np.uint32), hd[:whole].view(np.uint32)) and np.array_equal(gp[:whole].view(np.uint32), hp[:whole].view(np.uint32))
                assert np.all(np.diff(gd[whole:cap]) >= 0) and not (gd[whole:cap] == -7.0).any()
    # objects with __cuda_array_interface__ (what a torch tensor is to the mirror), offsets and total only
    from lidar_imu_init_amd.api import _DeviceFloat4
    d_o, d_t = _dev_filled(reg, np.full(n + 1, -7, np.int64)), _dev_filled(reg, np.full(1, -7, np.int64))
    reg.map_radius_dev(_DeviceFloat4(d_q, n), n, 1.0, d_o, None, None, 0, d_t, stride_bytes=16)
    ho = reg.map_radius(q, 1.0, points=False)[0]
    assert np.array_equal(_dev_array(reg, d_o, (n + 1,), "<i8"), ho) and _dev_array(reg, d_t, (1,), "<i8")[0] == ho[-1]


# ------------------------------------------------------------------------------------------------ 11. rules
def test_rules(small_world):
    import lidar_imu_init_amd as lii
    reg = lii.Registrar(max_scan_points=1000, max_map_points=100_000, filter_size_map=0.15)  # cell 0.45 m: max_dist up to (32 x 0.45)^2 = 207.36
    L, h = reg.L, reg.h
    q = np.ascontiguousarray(small_world_balls(small_world)[0][:50])
    n, cap = len(q), 16384
    sent = [np.full(n + 1, -7, np.int64), np.full((cap, 3), -7.0, np.float32), np.full(cap, -7.0, np.float32), np.full(1, -7, np.int64)]
    o, p, d, t = [a.copy() for a in sent]
    d_q = _dev_filled(reg, q)
    d_bufs = [_dev_filled(reg, a) for a in sent]

    def both(n_q, stride, md, flags=0, capacity=cap, qptr=True, optr=True, tptr=True):
        rc_h = L.lii_map_radius(h, q.ctypes.data if qptr else None, n_q, stride, C.c_double(md), flags, o.ctypes.data if optr else None, p.ctypes.data,
                                d.ctypes.data, capacity, t.ctypes.data if tptr else None)
        rc_d = L.lii_map_radius_dev(h, d_q if qptr else None, n_q, stride, C.c_double(md), flags, d_bufs[0] if optr else None, d_bufs[1], d_bufs[2], capacity,
                                    d_bufs[3] if tptr else None)
        reg.synchronize()
        return rc_h, rc_d

    def untouched():
        for a, s, addr in zip((o, p, d, t), sent, d_bufs):
            assert np.array_equal(a, s) and np.array_equal(_dev_array(reg, addr, s.shape, s.dtype.str), s)

    assert both(n, 12, 1.0) == (STATE, STATE) and b"no map" in L.lii_last_error(h)  # no map yet
    untouched()
    reg.map_build(np.ascontiguousarray(small_world[1], np.float32))
    for kw in (dict(md=float("nan")), dict(md=float("inf")), dict(md=-1.0), dict(md=-1e-300), dict(md=208.0), dict(stride=8), dict(stride=14), dict(n_q=-1),
               dict(flags=2), dict(flags=3), dict(flags=-1), dict(capacity=-1), dict(qptr=False), dict(optr=False), dict(tptr=False)):
        args = dict(n_q=n, stride=12, md=1.0)
        args.update(kw)
        assert both(**args) == (INVALID, INVALID), kw
        untouched()
    assert both(n, 12, 208.0) == (INVALID, INVALID) and b"0.450" in L.lii_last_error(h)  # the message names the cell size
    assert L.lii_map_radius(None, q.ctypes.data, n, 12, C.c_double(1.0), 0, o.ctypes.data, p.ctypes.data, d.ctypes.data, cap, t.ctypes.data) == INVALID
    untouched()
    # n = 0: LII_OK, offsets[0] = 0, total 0 - with and without queries
    for qptr in (True, False):
        o[0], t[0] = -7, -7
        reg.dev_upload(d_bufs[0], sent[0])
        reg.dev_upload(d_bufs[3], sent[3])
        assert both(0, 12, 1.0, qptr=qptr) == (0, 0)
        assert o[0] == 0 and t[0] == 0 and np.array_equal(o[1:], sent[0][1:]) and np.array_equal(p, sent[1]) and np.array_equal(d, sent[2])
        assert _dev_array(reg, d_bufs[0], (n + 1,), "<i8")[0] == 0 and _dev_array(reg, d_bufs[3], (1,), "<i8")[0] == 0
    # max_dist below 1 and 0 are served; the host and the device form agree
    for md in (0.0, 0.25):
        assert both(n, 12, md) == (0, 0)
        assert t[0] == o[n] <= cap and np.array_equal(_dev_array(reg, d_bufs[0], (n + 1,), "<i8"), o) and _dev_array(reg, d_bufs[3], (1,), "<i8")[0] == t[0]
        assert np.array_equal(_dev_array(reg, d_bufs[2], (cap,), "<f4")[:t[0]].view(np.uint32), d[:t[0]].view(np.uint32))
    assert t[0] > 0

    # from inside lii_scan_job::while_waiting: LII_ERR_STATE
    import bench
    seen = []

    def hook():
        tt, oo = C.c_int64(-7), np.full(n + 1, -7, np.int64)
        seen.append(L.lii_map_radius(h, q.ctypes.data, n, 12, C.c_double(1.0), 0, oo.ctypes.data, None, None, 0, C.byref(tt)))
        seen.append(L.lii_map_radius_dev(h, d_q, n, 12, C.c_double(1.0), 0, d_bufs[0], None, None, 0, d_bufs[3]))
        seen.append(int(tt.value == -7 and (oo == -7).all()))

    hall = small_world[0]
    scan, st = _scan_stream(hall, 0)
    prop = st.copy()
    reg2 = lii.Registrar(max_scan_points=40_000, max_map_points=400_000, filter_size_map=0.15)
    reg2.map_build(small_world[1])
    L, h = reg2.L, reg2.h
    d_q, d_bufs = _dev_filled(reg2, q), [_dev_filled(reg2, a) for a in sent]
    reg2.scan_register(st, prop, imu_poses=bench.pose_table(prop.rot_end, prop.pos_end), leaf=0.1, max_iterations=5, imu_en=True, scan_dev=reg2.device_scan(scan),
                       scan_sorted=True, while_waiting=hook)
    assert seen == [STATE, STATE, 1]
    reg2.close()
    reg.close()
