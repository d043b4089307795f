"""lii_map_nearest / lii_map_nearest_dev: KD_TREE::Nearest_Search for arbitrary points, k and max_dist on the device map.

Expected values: the float32 brute force of tests/map_nearest_cases.py (calc_dist's evaluation order), and the UNMODIFIED reference tree
where oracle/_ref is built - never the library.  d2 must be bit-equal for every query; points must be equal wherever no two d2 in the
list or at its edge are equal (tests/test_map_nearest_ref.py shows on the CPU that the reference tree meets the same brute force)."""
import ctypes as C

import numpy as np
import pytest

from map_nearest_cases import CASES, Brute, check_answer, d2_f32, small_world_brute

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5


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


def _same_as_tree(tree, q, k, max_dist, pts, d2, cnt, tied):
    """The library's answer against the reference tree's: counts, d2 bit for bit (the tree pads with inf, the library with 0), points where nothing is tied."""
    tp, td, tc = tree.knn(q, k=k, max_dist=max_dist, threads=3)
    rows = np.arange(k)[None, :] < tc[:, None]
    assert np.array_equal(cnt, tc)
    assert np.array_equal(np.where(rows, d2, 0).view(np.uint32), np.where(rows, td, 0).view(np.uint32))
    assert np.array_equal(pts[~tied], tp[~tied])


@pytest.mark.parametrize("k,max_dist", CASES)
def test_parity_with_brute_force_and_reference_tree(world_reg, world_ref, small_world, k, max_dist):
    q, brute = small_world_brute(small_world)
    pts, d2, cnt = world_reg.map_nearest(q, k=k, max_dist=max_dist)
    assert pts.shape == (len(q), k, 3) and d2.shape == (len(q), k) and cnt.shape == (len(q),)
    check_answer(brute, k, max_dist, pts, d2, cnt, "lii_map_nearest")
    assert cnt[-1] == 0 and cnt[-2] == 0  # the NaN query and the one at 1e7 m
    if world_ref is not None:
        _same_as_tree(world_ref, q, k, max_dist, pts, d2, cnt, brute.case(k, max_dist)[3])


def test_outputs_are_optional_and_strides_are_honoured(world_reg, small_world):
    """pts_out / d2_out may be NULL; queries at stride 16 and 48 give what the packed ones give; n beyond one chunk of rows."""
    q, brute = small_world_brute(small_world)
    L, h = world_reg.L, world_reg.h
    pts, d2, cnt = world_reg.map_nearest(q, k=5, max_dist=5.0)
    for width in (4, 12):
        wide = np.full((len(q), width), 7.0, np.float32)
        wide[:, :3] = q
        p2, e2, c2 = world_reg.map_nearest(wide, k=5, max_dist=5.0)
        assert wide.strides[0] == 4 * width and np.array_equal(c2, cnt) and np.array_equal(e2, d2) and np.array_equal(p2, pts)
    c3, d3 = np.zeros(len(q), np.int32), np.zeros((len(q), 5), np.float32)
    assert L.lii_map_nearest(h, q.ctypes.data, len(q), 12, 5, C.c_double(5.0), None, None, c3.ctypes.data) == 0 and np.array_equal(c3, cnt)
    assert L.lii_map_nearest(h, q.ctypes.data, len(q), 12, 5, C.c_double(5.0), None, d3.ctypes.data, c3.ctypes.data) == 0 and np.array_equal(d3, d2)
    # 70 000 queries x k = 64: five chunks of 16 384 queries
    rep = np.tile(q, (35, 1))
    pb, db, cb = world_reg.map_nearest(rep, k=64, max_dist=5.0)
    p1, d1, c1 = world_reg.map_nearest(q, k=64, max_dist=5.0)
    assert np.array_equal(cb, np.tile(c1, 35)) and np.array_equal(db, np.tile(d1, (35, 1))) and np.array_equal(pb, np.tile(p1, (35, 1, 1)))


def _map_points_at(brute, q, pts, d2, cnt):
    """every returned point is a map point at exactly the stated d2"""
    keys = {tuple(p) for p in brute.pts.tolist()}
    for i in range(len(q)):
        for j in range(cnt[i]):
            assert tuple(pts[i, j].tolist()) in keys
            assert d2_f32(q[i:i + 1], pts[i, j][None])[0, 0].view(np.uint32) == d2[i, j].view(np.uint32)


def test_crowded_cell_and_exact_ties():
    """One grid cell with 700 points, 40 of them exact duplicates of one position; queries inside the cell and on exact multiples of the
    cell size; k = 64 and k = 1."""
    import lidar_imu_init_amd as lii
    rng = np.random.default_rng(5)
    cs = 0.45  # 3 x filter_size_map
    cell_lo = np.array([4 * cs, -3 * cs, 2 * cs])
    crowd = (cell_lo + rng.uniform(0.02, cs - 0.02, (700, 3))).astype(np.float32)
    crowd[100:140] = crowd[100]
    pts = np.concatenate([crowd, rng.uniform(-6, 6, (2300, 3)).astype(np.float32)])
    reg = lii.Registrar(max_scan_points=5000, max_map_points=10_000, filter_size_map=0.15)
    reg.map_build(pts)
    assert reg.map_size() == 3000
    q = np.concatenate([
        (cell_lo + rng.uniform(0, cs, (40, 3))).astype(np.float32),
        crowd[100:101], crowd[[3, 650]],
        (np.round(rng.uniform(-8, 8, (40, 3))) * np.float32(cs)).astype(np.float32),  # on the cell faces, edges and corners
        np.array([cell_lo, cell_lo + cs, [0, 0, 0]], np.float32),
    ])
    brute = Brute(q, pts)
    for k, md in ((64, 1.0), (1, 1.0), (64, 30.0), (1, 5.0)):
        p, d, c = reg.map_nearest(q, k=k, max_dist=md)
        bc, bd, _, tied = brute.case(k, md)
        rows = np.arange(k)[None, :] < bc[:, None]
        print(f"crowded k={k} max_dist={md}: counts differ {int((c != bc).sum())}, tied queries {int(tied.sum())}")
        assert np.array_equal(c, bc)
        assert np.array_equal(np.where(rows, d, 0).view(np.uint32), np.where(rows, bd, 0).view(np.uint32))
        assert not d[~rows].any() and not p[~rows].any()
        _map_points_at(brute, q, p, d, c)
    # the query on the duplicated position: its 40 copies lead the list at d2 = 0
    p, d, c = reg.map_nearest(crowd[100:101], k=64, max_dist=1.0)
    assert c[0] == 64 and not d[0, :40].any() and d[0, 40] > 0 and np.array_equal(p[0, :40], np.tile(crowd[100], (40, 1)))
    reg.close()


def test_k_beyond_the_map():
    import lidar_imu_init_amd as lii
    rng = np.random.default_rng(8)
    pts = rng.uniform(-1, 1, (10, 3)).astype(np.float32)
    reg = lii.Registrar(max_scan_points=1000, max_map_points=1000, filter_size_map=0.15)
    reg.map_build(pts)
    q = np.array([[0, 0, 0], [0.5, -0.5, 0.2], [3.0, 0, 0]], np.float32)
    p, d, c = reg.map_nearest(q, k=64, max_dist=30.0)
    brute = Brute(q, pts)
    bc, bd, bi, _ = brute.case(64, 30.0)
    assert c.tolist() == [10, 10, 10] and np.array_equal(c, bc)
    assert np.all(np.diff(d[:, :10], axis=1) >= 0) and np.array_equal(d[:, :10], bd[:, :10]) and np.array_equal(p[:, :10], pts[bi[:, :10]])
    assert not d[:, 10:].any() and not p[:, 10:].any()
    reg.close()


def _check_against_download(reg, q, tree, what):
    """the query answers from the map AS IT IS: brute force over the downloaded map (and the reference tree fed the same operations)"""
    res = {(k, md): reg.map_nearest(q, k=k, max_dist=md) for k, md in ((5, 5.0), (16, 1.0), (64, 30.0))}
    now = reg.map_download()
    brute = Brute(q, now)
    for (k, md), (p, d, c) in res.items():
        check_answer(brute, k, md, p, d, c, what)
        if tree is not None:
            _same_as_tree(tree, q, k, md, p, d, c, brute.case(k, md)[3])
    return now


def test_a_map_that_has_changed(oracle):
    """After lii_map_add_points (down-sampled and not) and lii_map_delete_boxes the answers come from the map as it is."""
    import lidar_imu_init_amd as lii
    rng = np.random.default_rng(21)
    ds = 0.3
    base = np.c_[rng.uniform(-10, 10, (20_000, 2)), rng.normal(0, 0.03, 20_000)].astype(np.float32)
    reg = lii.Registrar(max_scan_points=30_000, max_map_points=100_000, filter_size_map=ds)
    tree = oracle.Tree("ref", downsample=ds) if oracle.ref_available() else None
    reg.map_build(base)
    if tree is not None:
        tree.build(base)
    q = np.concatenate([(base[rng.choice(len(base), 700)] + rng.normal(0, 0.1, (700, 3))), rng.uniform(-14, 14, (300, 3)) * [1, 1, 0.2]]).astype(np.float32)
    _check_against_download(reg, q, tree, "built")
    add = (base[rng.choice(len(base), 3000)] + rng.normal(0, 0.2, (3000, 3))).astype(np.float32)
    n_add = reg.map_add_points(add, True)
    if tree is not None:
        assert tree.add_points(add, True) == n_add
    _check_against_download(reg, q, tree, "after add_points(down-sampled)")
    # points the map did not have: a new patch beside it (new blocks of cells) and a cluster inside it
    plain = np.concatenate([rng.uniform([10.5, -3, -0.2], [13, 3, 0.2], (1500, 3)), rng.normal([1.0, 2.0, 0.3], 0.05, (500, 3))]).astype(np.float32)
    reg.map_add_points(plain, False)
    if tree is not None:
        tree.add_points(plain, False)
    now = _check_against_download(reg, q, tree, "after add_points(plain)")
    assert len(now) == reg.map_size()
    boxes = np.array([[-2, -2, -2, 2, 2, 2], [10, -10, -1, 14, 0, 1]], np.float32)
    n_del = reg.map_delete_boxes(boxes)
    assert n_del > 1000
    if tree is not None:
        assert tree.delete_boxes(boxes) == n_del
    now = _check_against_download(reg, q, tree, "after delete_boxes")
    assert not np.any(np.all((now >= boxes[0, :3]) & (now < boxes[0, 3:]), axis=1))
    reg.close()


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
    """lii_scan_job::map_update leaves the in-place update running behind the call; a query made right away joins it first."""
    import bench
    import lidar_imu_init_amd as lii
    hall, map_pts = small_world
    q, _ = small_world_brute(small_world)
    q = q[::4]
    reg = lii.Registrar(max_scan_points=40_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    n0 = reg.map_size()
    for k in range(2):
        scan, st = _scan_stream(hall, k)
        prop = st.copy()
        table = bench.pose_table(prop.rot_end, prop.pos_end)
        reg.scan_register(st, prop, imu_poses=table, leaf=0.1, max_iterations=5, imu_en=True, scan_dev=reg.device_scan(scan), scan_sorted=True, map_update=True)
        now = _check_against_download(reg, q, None, f"behind scan {k} with map_update")
    assert len(now) > n0  # the updates did add points
    reg.close()


def _dev_array(reg, addr, shape, typestr):
    """device memory -> numpy, through the runtime the library itself uses (symbols looked up through its own handle)"""
    hip = C.CDLL(reg.L._name)
    out = np.zeros(shape, np.dtype(typestr))
    reg.synchronize()
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(int(addr)), C.c_size_t(out.nbytes), C.c_int(2)) == 0  # hipMemcpyDeviceToHost
    return out


def test_device_form_equals_host_form(world_reg, small_world):
    q, _ = small_world_brute(small_world)
    reg, n = world_reg, len(q)
    wide = np.full((n, 4), 3.0, np.float32)  # stride 16: a float4 cloud
    wide[:, :3] = q
    d_q = reg.dev_alloc(wide.nbytes)
    reg._check(reg.L.lii_dev_upload(reg.h, d_q, wide.ctypes.data, wide.nbytes))
    for k, md in ((5, 5.0), (64, 30.0), (1, 1.0)):
        d_p, d_d, d_c = reg.dev_alloc(n * k * 12), reg.dev_alloc(n * k * 4), reg.dev_alloc(n * 4)
        reg.map_nearest_dev(d_q, n, k, md, d_p, d_d, d_c, stride_bytes=16)
        reg.synchronize()
        hp, hd, hc = reg.map_nearest(q, k=k, max_dist=md)
        assert np.array_equal(_dev_array(reg, d_c, (n,), "<i4"), hc)
        assert np.array_equal(_dev_array(reg, d_d, (n, k), "<f4").view(np.uint32), hd.view(np.uint32))
        assert np.array_equal(_dev_array(reg, d_p, (n, k, 3), "<f4"), hp)
    # objects with __cuda_array_interface__ (what a torch tensor is to the mirror), one output left out
    from lidar_imu_init_amd.api import _DeviceFloat, _DeviceFloat4
    d_d, d_c = reg.dev_alloc(n * 5 * 4), reg.dev_alloc(n * 4)
    reg.map_nearest_dev(_DeviceFloat4(d_q, n), n, 5, 5.0, None, _DeviceFloat(d_d, n * 5), _DeviceFloat(d_c, n), stride_bytes=16)
    hp, hd, hc = reg.map_nearest(q, k=5, max_dist=5.0)
    assert np.array_equal(_dev_array(reg, d_c, (n,), "<i4"), hc) and np.array_equal(_dev_array(reg, d_d, (n, 5), "<f4"), hd)


def _run_stream(small_world, with_queries):
    import bench
    import lidar_imu_init_amd as lii
    hall, map_pts = small_world
    q, _ = small_world_brute(small_world)
    reg = lii.Registrar(max_scan_points=40_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    states, reports, nbrs = [], [], []
    for k in range(3):
        scan, st = _scan_stream(hall, k)
        prop = st.copy()
        table = bench.pose_table(prop.rot_end, prop.pos_end)
        if with_queries:
            reg.map_nearest(q[:300], k=16, max_dist=5.0)
        rep = reg.scan_register(st, prop, imu_poses=table, leaf=0.1, max_iterations=5, imu_en=True, scan_dev=reg.device_scan(scan), scan_sorted=True,
                                map_update=(k == 1))
        if with_queries:
            reg.map_nearest(q, k=64, max_dist=30.0)  # (scan 1: its map update is still under way)
        nd = len(reg.scan_download(1))
        nbrs.append(reg.neighbors(nd))
        if k != 1:
            reg.map_incremental(st, want_counts=(k == 0))
            if with_queries:
                reg.map_nearest(q[:500], k=5, max_dist=1.0)  # (scan 2: the update runs beside it on its own stream)
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


def test_rules(small_world):
    import lidar_imu_init_amd as lii
    reg = lii.Registrar(max_scan_points=1000, max_map_points=100_000, filter_size_map=0.15)  # cell 0.45 m: max_dist up to (32 x 0.45)^2 = 207.36
    L, h = reg.L, reg.h
    q = np.ascontiguousarray(small_world_brute(small_world)[0][:50])
    n, k = len(q), 5
    sent_p, sent_d, sent_c = np.full((n, 64, 3), -7.0, np.float32), np.full((n, 64), -7.0, np.float32), np.full(n, -7, np.int32)
    p, d, c = sent_p.copy(), sent_d.copy(), sent_c.copy()
    d_bufs = [reg.dev_alloc(a.nbytes) for a in (q, p, d, c)]
    for a, addr in zip((q, p, d, c), d_bufs):
        reg._check(L.lii_dev_upload(h, addr, a.ctypes.data, a.nbytes))

    def both(n_q, stride, kk, md, qptr=True):
        rc_h = L.lii_map_nearest(h, q.ctypes.data if qptr else None, n_q, stride, kk, C.c_double(md), p.ctypes.data, d.ctypes.data, c.ctypes.data)
        rc_d = L.lii_map_nearest_dev(h, d_bufs[0] if qptr else None, n_q, stride, kk, C.c_double(md), d_bufs[1], d_bufs[2], d_bufs[3])
        reg.synchronize()
        return rc_h, rc_d

    def untouched():
        assert np.array_equal(p, sent_p) and np.array_equal(d, sent_d) and np.array_equal(c, sent_c)
        assert np.array_equal(_dev_array(reg, d_bufs[1], sent_p.shape, "<f4"), sent_p) and np.array_equal(_dev_array(reg, d_bufs[2], sent_d.shape, "<f4"), sent_d)
        assert np.array_equal(_dev_array(reg, d_bufs[3], sent_c.shape, "<i4"), sent_c)

    assert both(n, 12, k, 5.0) == (STATE, STATE) and b"no map" in L.lii_last_error(h)  # no map yet
    untouched()
    reg.map_build(np.ascontiguousarray(small_world[1], np.float32))
    for args in ((n, 12, 0, 5.0), (n, 12, 65, 5.0), (n, 12, -3, 5.0), (n, 12, k, 0.5), (n, 12, k, float("nan")), (n, 12, k, float("inf")), (n, 12, k, -1.0),
                 (n, 12, k, 208.0), (n, 8, k, 5.0), (n, 14, k, 5.0), (-1, 12, k, 5.0)):
        assert both(*args) == (INVALID, INVALID), args
        untouched()
    assert both(n, 12, k, 208.0) == (INVALID, INVALID) and b"0.450" in L.lii_last_error(h)  # the message names the cell size
    assert both(n, 12, k, 5.0, qptr=False) == (INVALID, INVALID)
    untouched()
    assert L.lii_map_nearest(h, q.ctypes.data, n, 12, k, C.c_double(5.0), p.ctypes.data, d.ctypes.data, None) == INVALID  # count is required
    assert L.lii_map_nearest(None, q.ctypes.data, n, 12, k, C.c_double(5.0), p.ctypes.data, d.ctypes.data, c.ctypes.data) == INVALID
    untouched()
    assert both(0, 12, k, 5.0) == (0, 0) and both(0, 12, k, 5.0, qptr=False) == (0, 0)  # n = 0
    untouched()
    assert both(n, 12, k, 207.0) == (0, 0)  # the largest ball this cell size takes
    assert (c > 0).any() and c.max() <= k and np.array_equal(_dev_array(reg, d_bufs[3], c.shape, "<i4"), c)
    reg.close()
