"""lii_map_surface / lii_map_surface_dev / lii_map_crispness: the ball of lii_map_radius reduced on the device to count, centroid,
covariance spectrum, normal and curvature, and the whole-map crispness figures.

Expected values: tests/map_surface_cases.py - the float32 brute-force balls of map_radius_cases.Balls, the relative moments in float64,
C by the header's formula, np.linalg.eigh - never the library.  Counts are compared exactly, everything else within the bounds DERIVED in
that module's docstring; tests/test_map_surface_ref.py shows on the CPU that the conditions these comparisons rely on hold."""
import ctypes as C

import numpy as np
import pytest

import map_surface_cases as msc
from map_nearest_cases import d2_f32
from map_radius_cases import Balls
from map_surface_cases import Surface, check_crispness, check_records, crispness_reference, sheet_map, small_world_crispness, small_world_surface

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5


@pytest.fixture(scope="module")
def world_reg(small_world):
    import lidar_imu_init_amd as lii
    reg = lii.Registrar(max_scan_points=10_000, max_map_points=100_000, filter_size_map=0.15)
    reg.map_build(np.ascontiguousarray(small_world[1], np.float32))
    yield reg
    reg.close()


def _small_reg(pts):
    import lidar_imu_init_amd as lii
    reg = lii.Registrar(max_scan_points=5000, max_map_points=20_000, filter_size_map=0.15)
    reg.map_build(pts)
    assert reg.map_size() == len(pts)
    return reg


def _dev_array(reg, addr, shape, dtype):
    """device memory -> numpy, through the runtime the library itself uses (symbols looked up through its own handle)"""
    hip = C.CDLL(reg.L._name)
    out = np.zeros(shape, dtype)
    reg.synchronize()
    if out.nbytes:
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(int(addr)), C.c_size_t(out.nbytes), C.c_int(2)) == 0  # hipMemcpyDeviceToHost
    return out


def _dev_filled(reg, a):
    addr = reg.dev_alloc(a.nbytes)
    reg.dev_upload(addr, a)
    return addr


def _bytes(rec):
    return np.ascontiguousarray(rec).view(np.uint8)


# ------------------------------------------------------------------------------------------------ 1. parity on small_world
@pytest.mark.parametrize("max_dist", msc.MAX_DISTS)
def test_parity_with_the_brute_force_reference(world_reg, small_world, max_dist):
    q, balls, refs = small_world_surface(small_world)
    rec = world_reg.map_surface(q, max_dist)
    left_out = check_records(rec, refs[max_dist], f"lii_map_surface max_dist={max_dist}")
    assert left_out <= 0.01 * refs[max_dist].valid.sum()
    assert not _bytes(rec[-2:]).any()  # the query at 1e7 m and the NaN query: count 0, valid 0, all zeros
    off = world_reg.map_radius(q, max_dist, points=False)[0]
    assert np.array_equal(rec["count"], np.diff(off))  # lii_map_radius's count, exactly


# ------------------------------------------------------------------------------------------------ 2. exact arithmetic
def test_exact_arithmetic_on_dyadic_lattices():
    """Coordinates at multiples of 2^-4: a plane, a line and a 3-D block, the queries on the same lattices.  Every moment is exactly
    representable, so the sums do not depend on their order: one dropped or doubled point anywhere shows in the bits."""
    import lidar_imu_init_amd as lii
    g = np.arange(-32, 33) / 16.0
    plane = np.array([[x, y, 1.5] for x in g for y in g])
    line = np.array([[x, 20.0, 0.0] for x in g])
    b = np.arange(-6, 7) / 16.0
    block = np.array([[-20.0 + x, y, -3.0 + z] for x in b for y in b for z in b])
    pts = np.concatenate([plane, line, block]).astype(np.float32)
    reg = _small_reg(pts)
    md = 0.25  # radius 0.5: 8 lattice steps, the points at exactly d2 == max_dist included
    q_plane = np.array([[0, 0, 1.5], [0.25, -0.5, 1.5], [-1.0, 1.0625, 1.5], [2.0, 2.0, 1.5], [0, 0, 1.5 + 1 / 16]], np.float32)  # (2, 2): the corner
    q_line = np.array([[0, 20.0, 0], [0.5, 20.0, 0], [2.0, 20.0, 0]], np.float32)
    q_block = np.array([[-20.0, 0, -3.0], [-20.0 + 6 / 16, 6 / 16, -3.0 - 6 / 16], [-20.0 + 1 / 16, 0, -3.0]], np.float32)
    q = np.concatenate([q_plane, q_line, q_block])
    ref = Surface(q, pts, Balls(q, pts, md).case(md), md)
    rec = reg.map_surface(q, md)
    print("counts", rec["count"].tolist(), "reference", ref.count.tolist())
    assert np.array_equal(rec["count"], ref.count) and np.array_equal(rec["valid"], ref.valid.astype(np.int32))
    assert np.array_equal(rec["mean"].view(np.uint64), ref.mean.view(np.uint64)), "a centroid differs in its bits"
    on = sum(1 for i in range(-8, 9) for j in range(-8, 9) if i * i + j * j <= 64)
    assert rec["count"][0] == rec["count"][1] == rec["count"][2] == on and rec["count"][5] == 17 and rec["count"][7] == 9
    # the plane, ball not cut: C is diagonal and exact - eig is its sorted diagonal bit for bit, eig[0] == 0, the normal is the z axis
    for k in (0, 1, 2):
        c6 = ref.c6[k]
        assert c6[1] == c6[2] == c6[4] == c6[5] == 0.0 and c6[0] == c6[3] > 0
        assert np.array_equal(rec["eig"][k].view(np.uint64), np.sort(c6[[0, 3, 5]]).view(np.uint64))
        assert np.array_equal(rec["eig"][k].view(np.uint64), np.maximum(lii.sym3_eigen(c6)[0], 0.0).view(np.uint64))
        assert rec["eig"][k][0] == 0.0 and rec["normal"][k].tolist() == [0.0, 0.0, 1.0] and rec["curvature"][k] == 0.0
    # the plane's corner and the query one step above it: cut or lifted balls, still flat - within the derived bounds
    check_records(rec, ref, "dyadic lattices", normals=False)
    for k in (3, 4):
        assert rec["eig"][k][0] <= ref.eig_bound()[k] and abs(abs(rec["normal"][k][2]) - 1.0) <= 1e-14
    # the line: two zero eigenvalues and a finite unit normal across it
    for k in (5, 6, 7):
        assert rec["valid"][k] == 1 and rec["eig"][k][0] == 0.0 and rec["eig"][k][1] == 0.0 and rec["eig"][k][2] == ref.c6[k][0] > 0
        nrm = rec["normal"][k]
        assert np.all(np.isfinite(nrm)) and abs(np.linalg.norm(nrm) - 1.0) <= 1e-14 and nrm[0] == 0.0
        assert rec["curvature"][k] == 0.0
    # the block's centre: a symmetric ball in three dimensions - an exact triple eigenvalue
    c6 = ref.c6[8]
    assert c6[0] == c6[3] == c6[5] > 0 and not c6[[1, 2, 4]].any()
    assert np.array_equal(rec["eig"][8], [c6[0]] * 3) and rec["curvature"][8] == c6[0] / (c6[0] + c6[0] + c6[0])
    # where C is not diagonal the device's solver and the host's run the same source on the same (exact) matrix
    same = [bool(np.array_equal(rec["eig"][k].view(np.uint64), np.maximum(lii.sym3_eigen(ref.c6[k])[0], 0.0).view(np.uint64))) for k in range(len(q))]
    print("device eig == lii_sym3_eigen(reference C), bit for bit:", same)
    reg.close()


# ------------------------------------------------------------------------------------------------ 3. batch edges in a crowded cell
def test_batch_edges_in_a_crowded_cell_and_the_inclusive_bound():
    """Balls of exactly 0, 1, 2, 3, 63, 64, 65, 128, 129 and 5 000 points, each inside one grid cell (the layout of
    test_gpu_map_radius.py's second test): the 64-point trip boundary and the lane-partial reduction.  A point at d2 == max_dist exactly
    is in, one at the next float above is out."""
    rng = np.random.default_rng(11)
    cs = 0.45
    pops = (0, 1, 2, 3, 63, 64, 65, 128, 129, 5000)
    centres = np.array([[(8 * i + 4.5) * cs, 20.5 * cs, -7.5 * cs] for i in range(len(pops))])  # cell centres, 8 cells apart
    clouds = [(c + rng.uniform(-0.1, 0.1, (p, 3))).astype(np.float32) for c, p in zip(centres, pops)]  # all within sqrt(0.03) < 0.2 m
    y = np.float32(2.0 ** -11.5)
    edge = np.array([[1, 0, 0], [0, 1, y]], np.float32)  # d2 from the origin: 1 exactly, and the next float above 1
    pts = np.concatenate(clouds + [edge, rng.uniform(-12, -2, (2000, 3)).astype(np.float32)])
    reg = _small_reg(pts)
    q = centres.astype(np.float32)
    rec = reg.map_surface(q, 0.04)
    assert rec["count"].tolist() == list(pops)
    ref = Surface(q, pts, Balls(q, pts, 0.04).case(0.04), 0.04)
    print("gaps", np.round(ref.gap(), 4).tolist())
    check_records(rec, ref, "crowded cells")
    for md in (1.0, 3.0):  # wider balls over the same map (the crowded cells among their neighbours)
        check_records(reg.map_surface(q, md), Surface(q, pts, Balls(q, pts, md).case(md), md), f"crowded cells, max_dist={md}")
    origin = np.zeros((1, 3), np.float32)
    above = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    d = np.sort(d2_f32(origin, pts)[0])
    assert d[0] == 1.0 and float(d[1]) == above and d[2] > 2.0
    r = reg.map_surface(origin, 1.0)[0]
    assert r["count"] == 1 and r["valid"] == 0 and r["mean"].tolist() == [1.0, 0.0, 0.0] and not r["eig"].any() and not r["normal"].any()
    assert reg.map_surface(origin, float(np.nextafter(1.0, 0.0)))["count"][0] == 0
    assert reg.map_surface(origin, above)["count"][0] == 2
    assert reg.map_surface(origin, float(np.nextafter(above, 0.0)))["count"][0] == 1
    reg.close()


# ------------------------------------------------------------------------------------------------ 4. determinism and forms
def test_determinism_and_forms(world_reg, small_world):
    q, balls, refs = small_world_surface(small_world)
    reg, n, md = world_reg, len(q), 0.25
    host = reg.map_surface(q, md)
    assert np.array_equal(_bytes(host), _bytes(reg.map_surface(q, md)))  # two calls
    i = int(np.argmax(refs[md].count))  # the fullest ball: two trips and a partial one
    assert refs[md].count[i] > 64
    alone = reg.map_surface(q[i:i + 1], md)
    seven = reg.map_surface(q[[3, 900, i, 1999, 1998, 5, 1200]], md)
    big = np.tile(q, (33, 1))[:65_537].copy()
    big[65_536] = q[i]  # behind the host form's chunk of 65 536 queries
    many = reg.map_surface(big, md)
    assert len(_bytes(alone)) == 88
    assert np.array_equal(_bytes(alone), _bytes(host[i:i + 1])) and np.array_equal(_bytes(alone), _bytes(seven[2:3]))
    assert np.array_equal(_bytes(alone), _bytes(many[65_536:]))
    assert np.array_equal(_bytes(many[:n]), _bytes(host)) and np.array_equal(_bytes(many[n:2 * n]), _bytes(host))
    # the device form, stride 16
    wide = np.full((n, 4), 3.0, np.float32)
    wide[:, :3] = q
    d_q, d_out = _dev_filled(reg, wide), _dev_filled(reg, np.full(88 * n, 7, np.uint8))
    reg.map_surface_dev(d_q, n, md, d_out, stride_bytes=16)
    assert np.array_equal(_dev_array(reg, d_out, (88 * n,), np.uint8), _bytes(host))
    # with a viewpoint: every valid normal looks at it and is +- the unoriented one
    vp = np.array([1.0, -2.0, 1.5])
    seen = reg.map_surface(q, md, viewpoint=vp)
    reg.map_surface_dev(d_q, n, md, d_out, viewpoint=vp, stride_bytes=16)
    assert np.array_equal(_dev_array(reg, d_out, (88 * n,), np.uint8), _bytes(seen))
    v = host["valid"] == 1
    assert v.sum() > 1000
    for f in ("count", "valid", "mean", "eig", "curvature"):
        assert np.array_equal(seen[f], host[f])
    dot = np.einsum("ij,ij->i", seen["normal"][v], vp[None] - seen["mean"][v])
    assert np.all(dot >= 0.0)
    sign = np.where(np.all(seen["normal"][v] == host["normal"][v], axis=1), 1.0, -1.0)
    assert np.array_equal(seen["normal"][v], host["normal"][v] * sign[:, None]) and (sign < 0).any() and (sign > 0).any()
    # without one: the component of largest magnitude is positive
    nv = host["normal"][v]
    assert np.all(nv[np.arange(len(nv)), np.argmax(np.abs(nv), axis=1)] > 0)
    assert not seen["normal"][~v].any()


# ------------------------------------------------------------------------------------------------ 5. observer, rules
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


def _run_stream(small_world, with_queries):
    import bench
    import lidar_imu_init_amd as lii
    hall, map_pts = small_world
    q = small_world_surface(small_world)[0]
    reg = lii.Registrar(max_scan_points=40_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    d_q, d_out = _dev_filled(reg, np.ascontiguousarray(q[:200])), reg.dev_alloc(200 * 88)
    states, reports, nbrs, sizes = [], [], [], []
    for k in range(3):
        scan, st = _scan_stream(hall, k)
        prop = st.copy()
        table = bench.pose_table(prop.rot_end, prop.pos_end)
        if with_queries:
            reg.map_surface(q[:300], 0.25)
        rep = reg.scan_register(st, prop, imu_poses=table, leaf=0.1, max_iterations=5, imu_en=True, scan_dev=reg.device_scan(scan), scan_sorted=True,
                                map_update=(k == 1))
        if with_queries:
            reg.map_surface(q[::5], 1.0, viewpoint=[0.0, 0.0, 1.0])  # (scan 1: its map update is still under way)
            reg.map_crispness(0.25, every=16)
        nd = len(reg.scan_download(1))
        nbrs.append(reg.neighbors(nd))
        if k != 1:
            reg.map_incremental(st, want_counts=(k == 0))
            if with_queries:
                reg.map_surface_dev(d_q, 200, 1.0, d_out)  # (scan 2: the update runs beside it on its own stream)
                reg.map_crispness(0.04, min_count=4, every=64)
        sizes.append(reg.map_size())
        states.append(st.pod.copy())
        reports.append([rep["iterations"], rep["searches"], rep["effect_num"], int(rep["converged"])] + list(rep["normal_eq"]))
    final = reg.map_download()
    reg.close()
    return np.array(states), np.array(reports), nbrs, final[np.lexsort(final.T)], sizes


def test_surface_calls_do_not_disturb_a_registration_stream(small_world):
    """Two handles run the same 3-scan stream; one is asked for surfaces and crispness between the scans.  States, reports, neighbour
    lists, map sizes and map sets are equal."""
    a = _run_stream(small_world, False)
    b = _run_stream(small_world, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]) and a[4] == b[4]
    for (pa, ca, sa), (pb, cb, sb) in zip(a[2], b[2]):
        assert np.array_equal(ca, cb) and np.array_equal(sa, sb) and np.array_equal(pa, pb)


def test_rules(small_world):
    import bench
    import lidar_imu_init_amd as lii
    from lidar_imu_init_amd import api
    reg = lii.Registrar(max_scan_points=1000, max_map_points=100_000, filter_size_map=0.15)  # cell 0.45 m: max_dist up to (32 x 0.45)^2 = 207.36
    L, h = reg.L, reg.h
    q = np.ascontiguousarray(small_world_surface(small_world)[0][:50])
    n = len(q)
    sent = np.full(88 * n, 7, np.uint8)
    out = sent.copy()
    d_q, d_out = _dev_filled(reg, q), _dev_filled(reg, sent)
    cr = api.lii_map_crispness(7, 7, 7, 7, 7.0, 7.0, 7.0)

    def both(n_q=n, stride=12, md=1.0, qptr=True, optr=True):
        rc_h = L.lii_map_surface(h, q.ctypes.data if qptr else None, n_q, stride, C.c_double(md), None, out.ctypes.data if optr else None)
        rc_d = L.lii_map_surface_dev(h, d_q if qptr else None, n_q, stride, C.c_double(md), None, d_out if optr else None)
        reg.synchronize()
        return rc_h, rc_d

    def untouched():
        assert np.array_equal(out, sent) and np.array_equal(_dev_array(reg, d_out, sent.shape, np.uint8), sent)
        assert (cr.n_selected, cr.n_used, cr.n_sparse, cr.n_degenerate, cr.mme, cr.mpv, cr.mean_count) == (7, 7, 7, 7, 7.0, 7.0, 7.0)

    assert both() == (STATE, STATE) and b"no map" in L.lii_last_error(h)  # no map yet
    assert L.lii_map_crispness(h, 0.25, 5, 1, C.byref(cr)) == STATE
    untouched()
    assert both(n_q=0) == (0, 0) and both(n_q=0, qptr=False, optr=False) == (0, 0)  # n == 0: LII_OK, map or not
    reg.map_build(np.ascontiguousarray(small_world[1], np.float32))
    for kw in (dict(md=float("nan")), dict(md=float("inf")), dict(md=-1.0), dict(md=-1e-300), dict(md=208.0), dict(stride=8), dict(stride=14), dict(n_q=-1),
               dict(qptr=False), dict(optr=False)):
        assert both(**kw) == (INVALID, INVALID), kw
        untouched()
    assert both(md=208.0) == (INVALID, INVALID) and b"0.450" in L.lii_last_error(h)  # the message names the cell size
    for md, mc, ev, ptr in ((float("nan"), 5, 1, True), (float("inf"), 5, 1, True), (-1.0, 5, 1, True), (208.0, 5, 1, True), (0.25, 3, 1, True), (0.25, 5, 0, True),
                            (0.25, 5, -1, True), (0.25, 5, 1, False)):
        assert L.lii_map_crispness(h, C.c_double(md), mc, ev, C.byref(cr) if ptr else None) == INVALID, (md, mc, ev, ptr)
        untouched()
    assert both(n_q=0) == (0, 0)
    untouched()
    # served: max_dist 0 and the largest ball; the host and the device form agree
    for md in (0.0, 0.25, 207.36):
        m = 4 if md > 100 else n
        assert both(n_q=m, md=md) == (0, 0)
        assert np.array_equal(_dev_array(reg, d_out, sent.shape, np.uint8)[:88 * m], out[:88 * m])
        rec = out[:88 * m].view(api.SURFACE_DTYPE)
        assert np.array_equal(rec["count"], np.diff(reg.map_radius(q[:m], md, points=False)[0]))
    assert rec["count"].max() > 10_000  # balls of radius 14.4 m: most of the hall
    assert L.lii_map_crispness(h, 0.25, 4, 1000, C.byref(cr)) == 0 and 0 < cr.n_selected < 300

    # from inside lii_scan_job::while_waiting: LII_ERR_STATE
    seen = []
    scan, st = _scan_stream(small_world[0], 0)
    prop = st.copy()
    reg2 = lii.Registrar(max_scan_points=40_000, max_map_points=400_000, filter_size_map=0.15)
    reg2.map_build(small_world[1])
    L2, h2 = reg2.L, reg2.h
    d_q2, d_out2 = _dev_filled(reg2, q), _dev_filled(reg2, sent)
    out2, cr2 = sent.copy(), api.lii_map_crispness(7, 7, 7, 7, 7.0, 7.0, 7.0)

    def hook():
        seen.append(L2.lii_map_surface(h2, q.ctypes.data, n, 12, C.c_double(1.0), None, out2.ctypes.data))
        seen.append(L2.lii_map_surface_dev(h2, d_q2, n, 12, C.c_double(1.0), None, d_out2))
        seen.append(L2.lii_map_crispness(h2, C.c_double(0.25), 5, 16, C.byref(cr2)))

    reg2.scan_register(st, prop, imu_poses=bench.pose_table(prop.rot_end, prop.pos_end), leaf=0.1, max_iterations=5, imu_en=True, scan_dev=reg2.device_scan(scan),
                       scan_sorted=True, while_waiting=hook)
    assert seen == [STATE, STATE, STATE] and np.array_equal(out2, sent) and cr2.n_selected == 7
    assert np.array_equal(_dev_array(reg2, d_out2, sent.shape, np.uint8), sent)
    reg2.close()
    reg.close()


# ------------------------------------------------------------------------------------------------ 6. crispness
def test_crispness(world_reg, small_world):
    expected, bounds, _ = small_world_crispness(small_world)
    got = world_reg.map_crispness(**msc.CRISP_WORLD)
    check_crispness(got, expected, bounds, "small_world, every 16")
    assert got == world_reg.map_crispness(**msc.CRISP_WORLD)  # identical bits on every call
    assert 3000 < got["n_selected"] < 6000

    figures = {}
    for noise in (0.0, 0.03):
        pts = sheet_map(noise=noise)
        reg = _small_reg(pts)
        exp, bnd, ref = crispness_reference(pts, 0.25, 5, 1)
        got = reg.map_crispness(0.25, min_count=5, every=1)
        check_crispness(got, exp, bnd, f"sheets, noise {noise}")
        assert (got["n_selected"], got["n_sparse"], got["n_degenerate"]) == (len(pts), 40, 9)
        assert got == reg.map_crispness(0.25, 5, 1)
        figures[noise] = got
        if noise == 0.0:
            # half of it removed: the figures follow the reference on the points that remain
            assert reg.map_delete_boxes(np.array([[-50, -50, -50, 0, 50, 50]], np.float32)) > 2000
            now = reg.map_download()
            assert len(now) == reg.map_size() < len(pts)
            for every in (1, 4):
                exp, bnd, _ = crispness_reference(now, 0.25, 5, every)
                check_crispness(reg.map_crispness(0.25, 5, every), exp, bnd, f"sheets after delete_boxes, every {every}")
        reg.close()
    print("flat", figures[0.0], "\n3 cm", figures[0.03])
    assert figures[0.03]["mme"] > figures[0.0]["mme"] and figures[0.03]["mpv"] > figures[0.0]["mpv"]  # what the figures are for
