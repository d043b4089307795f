"""The time sort of a scan on the device - lii_scan_sort and lii_scan_job::scan_sorted = 2 (lii_scan.hip: k_sort_keys / k_sort_gather
around the stable radix sort of lii_sort.hip) - against the oracle's sort_by_time (oracle/orc_scan.hpp:40-44: ascending t, compared as
floats, stable), which is the order the reference gives every scan before it de-skews it (src/IMU_Processing.hpp:209, :287).

Every comparison is bit for bit (the float32 words as uint32): a sort moves points, it computes nothing.  The one tolerance, 1e-5 m in
test 3, is the issue's: a scan registered in input order differs from the reference's cloud by the rounding of the voxel sums only.

The pose table of the lii_scan_register cases has ZERO angular rate (the platform translates and accelerates): the device's de-skew is
held to 2 float ulp against the oracle's, not to its bits, because device sin / cos and glibc's differ in the last double bit
(tests/test_gpu_scan_ops.py); without a rotation inside the sweep Exp() is the identity on both sides and test 3 can ask for the bits
of the whole chain.  The lii_scan_register_imu / _cv cases rotate; they compare two GPU runs."""
import ctypes as C

import numpy as np
import pytest

from harness import synth, wire

pytestmark = pytest.mark.gpu

LEAF, MAX_IT = 0.2, 5
RINGS, COLS = 16, 256
T_BEG = 100.0
_cache = {}


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _world():
    """A small room, its map (a few thousand points), a ring-major scan of 16 x 256 rays (one stamp per column: every stamp is shared
    by up to 16 points, and the input order is about as far from the time order as it gets), a state near the truth."""
    if "world" not in _cache:
        from oracle import oracle as O
        hall = synth.Hall(size=(8.0, 6.0, 3.5), n_boxes=2, seed=7)
        map_pts = hall.surface_points(0.2, noise=0.01, seed=7)
        R, p = synth.rot_zyx(0.01, -0.02, 0.3), np.array([0.3, -0.2, 0.1])
        dirs, t_ms = synth.spinning_lidar(RINGS, COLS, -15.0, 15.0)  # ring-major
        rng = np.random.default_rng(12)
        r = hall.raycast(p, dirs @ R.T) + rng.normal(0, 0.01, len(dirs))
        ok = np.isfinite(r) & (r > 0.5)
        scan = np.ascontiguousarray(np.c_[dirs[ok] * r[ok, None], t_ms[ok]], np.float32)
        st = O.state_init()
        v = O.StateView(st)
        v.rot_end[:] = R
        v.pos_end[:] = p
        st0 = O.state_boxplus(st, np.r_[0.002, -0.001, 0.002, 0.01, -0.01, 0.005, np.zeros(18)])
        _cache["world"] = (hall, map_pts, scan, R, p, st0)
    return _cache["world"]


def _pose_table(s0):
    """IMUpose of a platform that translates and accelerates without turning (see the module's docstring)."""
    import lidar_imu_init_amd as lii
    T = lii.pose6d_array(6)
    for k in range(6):
        t = 0.02 * k
        T[k, 0] = t
        T[k, 1:4] = [0.4, -0.3, 0.2]   # acc
        T[k, 4:7] = 0.0                # gyr
        T[k, 7:10] = np.array([0.5, -0.2, 0.1]) + np.array([0.4, -0.3, 0.2]) * t
        T[k, 10:13] = s0.pos_end + np.array([0.5, -0.2, 0.1]) * (t - 0.1)
        T[k, 13:22] = s0.rot_end.reshape(-1)
    return T


def _registrar(n_map, **kw):
    import lidar_imu_init_amd as lii
    return lii.Registrar(**{**dict(max_scan_points=5000, max_map_points=max(2 * n_map, 1000), filter_size_map=0.2), **kw})


def _imu_feed(R):
    """Twenty 200 Hz samples over the sweep of a platform that turns slowly; the carry of the scan before."""
    t = T_BEG + 0.005 * np.arange(1, 21)
    rows = np.c_[t, np.tile([0.02, -0.03, 0.05], (20, 1)), np.tile(R.T @ np.array([0.0, 0.0, 9.81]), (20, 1))]
    carry = dict(last_imu=np.r_[T_BEG - 0.001, rows[0, 1:]], acc_s_last=np.zeros(3), angvel_last=np.zeros(3), last_lidar_end_time=T_BEG)
    return rows, carry


def _results(reg, state, rep):
    n_body = len(reg.scan_download(1))
    nb, cnt, sel = reg.neighbors(n_body)
    return dict(state=state.pod.copy(), rep=(rep["iterations"], rep["searches"], rep["effect_num"]), scan=reg.scan_download(0),
                body=reg.scan_download(1), nb=nb, cnt=cnt, sel=sel)


def _same(a, b, what):
    assert a["rep"] == b["rep"], (what, a["rep"], b["rep"])
    assert np.array_equal(a["state"].view(np.uint64), b["state"].view(np.uint64)), f"{what}: final state / covariance"
    for k in ("scan", "body", "nb"):
        assert a[k].shape == b[k].shape and np.array_equal(_u32(a[k]), _u32(b[k])), f"{what}: {k}"
    assert np.array_equal(a["cnt"], b["cnt"]) and np.array_equal(a["sel"], b["sel"]), f"{what}: neighbour counts / selection"


def _register(path, scan, scan_sorted, *, scan_dev=False, next_scan=False, reg=None):
    """One registration of `scan` on a fresh handle (or on `reg`) through lii_scan_register ("poses"), _imu or _cv."""
    import lidar_imu_init_amd as lii
    hall, map_pts, _, R, p, st0 = _world()
    own = reg is None
    if own:
        reg = _registrar(len(map_pts))
        reg.map_build(map_pts)
    dev = reg.device_scan(scan) if (scan_dev or next_scan) else None
    if not scan_dev:
        reg.scan_upload(scan)
    kw = dict(leaf=LEAF, max_iterations=MAX_IT, scan_sorted=scan_sorted, scan_dev=dev if scan_dev else None)
    s0 = lii.State(st0)
    if path == "poses":
        st = s0.copy()
        rep = reg.scan_register(st, s0, imu_poses=_pose_table(s0), imu_en=False, next_scan=dev if next_scan else None, **kw)
    elif path == "imu":
        rows, carry = _imu_feed(R)
        reg.set_imu_noise(cov_gyr=0.1, cov_acc=0.1, mean_acc_norm=9.81)
        reg.imu_carry = carry
        s0.gravity[:] = [0.0, 0.0, -9.81]
        s0.cov[:] = np.diag(np.r_[np.full(6, 1e-4), np.full(6, 1e-4), np.full(3, 1e-2), np.full(9, 1e-5)])
        st, _, rep = reg.register_imu(rows, T_BEG, s0.copy(), imu_en=True, next_scan=dev if next_scan else None, **kw)
    else:
        s0.bias_g[:] = [0.02, -0.03, 0.05]
        s0.vel_end[:] = [0.3, -0.1, 0.05]
        st, _, rep = reg.register_cv(0.1, np.full(3, 50.0), np.full(3, 2.0), s0.copy(), **kw)
    out = _results(reg, st, rep)
    out["dev"] = dev
    if own:
        reg.close()
    return out


# ------------------------------------------------------------------------------------------------ 1. lii_scan_sort vs the oracle
def _stamps(pattern, n, rng):
    if pattern == "distinct":
        return rng.permutation(n).astype(np.float32) * np.float32(0.037)
    if pattern == "seven":
        return rng.choice(np.array([0.0, 1.5, 3.25, 7.0, 20.0, 55.5, 99.0], np.float32), n)
    if pattern == "equal":
        return np.full(n, 42.5, np.float32)
    if pattern == "ascending":
        return np.arange(n, dtype=np.float32) * np.float32(0.01)
    if pattern == "descending":
        return np.arange(n, dtype=np.float32)[::-1] * np.float32(0.01)
    if pattern == "zeros":  # -0.0 and +0.0 are EQUAL stamps; negative stamps; a denormal
        pool = np.array([-0.0, 0.0, -0.0, 0.0, -1.5, -1e-3, 1e-42, -1e-42, 2.0, 0.25], np.float32)
        return pool[rng.integers(0, len(pool), n)] if n > 2 else pool[:n][::-1].copy()
    raise AssertionError(pattern)


@pytest.fixture(scope="module")
def sorter():
    import lidar_imu_init_amd as lii
    r = lii.Registrar(max_scan_points=5000, max_map_points=1000, filter_size_map=0.2)
    yield r
    r.close()


@pytest.mark.parametrize("pattern", ["distinct", "seven", "equal", "ascending", "descending", "zeros", "ring_major"])
def test_scan_sort_equals_the_oracle_bit_for_bit(sorter, oracle, pattern):
    rng = np.random.default_rng(5)
    sizes = [RINGS * 64] if pattern == "ring_major" else [1, 2, 5, 64, 65, 257, 1000, 4099]
    for n in sizes:
        pts = np.zeros((n, 4), np.float32)
        pts[:, :3] = rng.normal(0, 5, (n, 3))
        pts[:, 0] = np.arange(n)  # (which input point is which: the stable order shows)
        if pattern == "ring_major":
            pts[:, 3] = np.tile(np.arange(64, dtype=np.float32) * np.float32(100.0 / 64), RINGS)
        else:
            pts[:, 3] = _stamps(pattern, n, rng)
        ref = oracle.sort_by_time(pts)
        if pattern == "zeros" and n >= 64:
            assert np.signbit(ref[ref[:, 3] == 0, 3]).any() and not np.signbit(ref[ref[:, 3] == 0, 3]).all()
            z = ref[ref[:, 3] == 0, 0]
            assert np.all(np.diff(z) > 0)  # (the oracle keeps -0.0 and +0.0 in input order)
        sorter.scan_upload(pts)
        sorter.scan_sort()
        got = sorter.scan_download(0)
        assert got.shape == ref.shape
        assert np.array_equal(_u32(got), _u32(ref)), f"{pattern} n={n}: first difference at row {int(np.argmax((_u32(got) != _u32(ref)).any(axis=1)))}"
        # sorting again changes nothing, and the other sources of a current scan sort alike
        sorter.scan_sort()
        assert np.array_equal(_u32(sorter.scan_download(0)), _u32(ref))
    dev = sorter.device_scan(pts)
    sorter.scan_set_device(dev)
    sorter.scan_sort()
    assert np.array_equal(_u32(sorter.scan_download(0)), _u32(ref))
    sorter.scan_upload_next(pts)
    sorter.scan_advance()
    sorter.scan_sort()
    assert np.array_equal(_u32(sorter.scan_download(0)), _u32(ref))


def test_scan_sort_with_nan_stamps_keeps_every_point(sorter):
    """A NaN stamp is outside the contract - any order - but every input point appears exactly once."""
    rng = np.random.default_rng(9)
    n = 1000
    pts = rng.normal(0, 5, (n, 4)).astype(np.float32)
    pts[:, 0] = np.arange(n)
    pts[rng.random(n) < 0.1, 3] = np.nan
    pts[7, 3] = -np.nan
    sorter.scan_upload(pts)
    sorter.scan_sort()
    got = sorter.scan_download(0)
    order = np.argsort(got[:, 0], kind="stable")
    assert np.array_equal(_u32(got[order]), _u32(pts))
    fin = got[np.isfinite(got[:, 3]), 3]
    assert np.all(np.diff(fin) >= 0)  # (the finite stamps still ascend among themselves: NaN keys sort to the two ends)


# ------------------------------------------------------------------------------------------------ 2. sorting registration == pre-sorted one
@pytest.mark.parametrize("scan_dev", [False, True])
@pytest.mark.parametrize("path", ["poses", "imu", "cv"])
def test_sorting_registration_equals_the_presorted_one(oracle, path, scan_dev):
    _, _, scan, _, _, _ = _world()
    assert len(np.unique(scan[:, 3])) < len(scan) / 8 and np.any(np.diff(scan[:, 3]) < 0)  # ties, and not in order
    a = _register(path, scan, 2, scan_dev=scan_dev)
    b = _register(path, oracle.sort_by_time(scan), 1, scan_dev=scan_dev)
    print(f"{path} scan_dev={scan_dev}: report {a['rep']}, {len(a['body'])} of {len(scan)} points behind the filter")
    assert a["rep"][2] > 200
    _same(a, b, f"{path}: scan_sorted = 2 against the host-sorted scan with scan_sorted = 1")
    if path == "poses" and not scan_dev:
        _cache["poses_sorted2"] = a


# ------------------------------------------------------------------------------------------------ 3. the reference's bits
def test_sorting_registration_gives_the_reference_cloud(oracle):
    import lidar_imu_init_amd as lii
    _, _, scan, _, _, st0 = _world()
    s0 = lii.State(st0)
    T = _pose_table(s0)
    # the oracle alone, on the CPU: the reference's chain (it sorts inside), and the same points summed in INPUT order
    ref_scan = oracle.undistort_imu(scan, T, s0.rot_end, s0.pos_end, s0.offset_R_L_I, s0.offset_T_L_I)
    ref_body, filtered = oracle.voxel_grid(ref_scan, LEAF)
    perm = np.argsort(scan[:, 3], kind="stable")  # (stamps >= 0: no signed zero to tell apart)
    assert np.array_equal(_u32(scan[perm]), _u32(oracle.sort_by_time(scan)))
    unsorted = np.empty_like(ref_scan)
    unsorted[perm] = ref_scan
    body_in_order, _ = oracle.voxel_grid(unsorted, LEAF)
    vox = np.floor(ref_scan[:, :3] / np.float32(LEAF)).astype(np.int64)
    _, inv, cnt = np.unique(vox, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    crowded = [v for v in np.nonzero(cnt >= 3)[0] if len(np.unique(ref_scan[inv == v, 3])) >= 2]
    flipped = int((_u32(body_in_order) != _u32(ref_body)).any(axis=1).sum())
    print(f"oracle: {len(ref_body)} voxels, {len(crowded)} hold >= 3 points with different stamps; input order changes {flipped} centroids")
    assert filtered and len(crowded) >= 5
    assert body_in_order.shape == ref_body.shape and flipped >= 1  # reordering changes a float sum
    # the device
    a = _cache.get("poses_sorted2") or _register("poses", scan, 2)
    d_scan = int((_u32(a["scan"]) != _u32(ref_scan)).sum())
    print(f"scan_sorted = 2: de-skewed scan differs from the oracle's in {d_scan} words, down-sampled cloud in "
          f"{int((_u32(a['body']) != _u32(ref_body)).sum()) if a['body'].shape == ref_body.shape else -1} words")
    assert a["body"].shape == ref_body.shape
    assert np.array_equal(_u32(a["body"]), _u32(ref_body)), "scan_sorted = 2 must give the reference's down-sampled cloud, bit for bit"
    plain = _register("poses", scan, 0)
    assert plain["body"].shape == ref_body.shape
    n_diff = int((_u32(plain["body"]) != _u32(ref_body)).sum())
    d_max = float(np.abs(plain["body"][:, :3].astype(np.float64) - ref_body[:, :3]).max())
    print(f"scan_sorted = 0: {n_diff} words differ from the reference's cloud, max |d| {d_max:.2e} m")
    assert n_diff >= 1
    assert d_max <= 1e-5


# ------------------------------------------------------------------------------------------------ 4. the whole-message ingest
def test_whole_message_frame_registers_with_the_reference_bits(oracle):
    import lidar_imu_init_amd as lii
    hall, map_pts, _, R, p, st0 = _world()
    dirs, t_ms = synth.spinning_lidar(RINGS, 128, -15.0, 15.0)  # ring-major, as an Ouster driver publishes it
    rng = np.random.default_rng(3)
    r = hall.raycast(p, dirs @ R.T) + rng.normal(0, 0.01, len(dirs))
    xyz = (dirs * r[:, None]).astype(np.float32)
    ring = (np.arange(len(xyz)) // 128).astype(np.int32)
    raw = wire.pack_pcl2(wire.OUSTER, xyz, ring, t_ms.astype(np.float64), T_BEG)
    f = wire.pc2_fields(wire.OUSTER)
    args = (raw, len(xyz), f, wire.OUSTER, RINGS, 1, 0.5, T_BEG, 0, 100)
    orc = oracle.ingest_pcl2(*args)
    assert len(orc) == 1
    frame = orc[0][1]
    assert len(frame) > 1500 and np.any(np.diff(frame[:, 3]) < 0)  # input order, not time order
    s0 = lii.State(st0)
    T = _pose_table(s0)
    ref_scan = oracle.undistort_imu(oracle.sort_by_time(frame), T, s0.rot_end, s0.pos_end, s0.offset_R_L_I, s0.offset_T_L_I)
    ref_body, _ = oracle.voxel_grid(ref_scan, LEAF)
    reg = _registrar(len(map_pts))
    reg.map_build(map_pts)
    info = reg.ingest_pcl2(*args)
    assert len(info) == 1 and info[0][2] == len(frame)
    reg.frame_select(0)
    st = s0.copy()
    rep = reg.scan_register(st, s0, imu_poses=T, leaf=LEAF, max_iterations=MAX_IT, imu_en=False, scan_sorted="sort")
    assert rep["effect_num"] > 200
    got_scan, got_body = reg.scan_download(0), reg.scan_download(1)
    assert got_scan.shape == ref_scan.shape and np.array_equal(_u32(got_scan), _u32(ref_scan))
    assert got_body.shape == ref_body.shape and np.array_equal(_u32(got_body), _u32(ref_body))
    # the frame itself was only read
    reg.frame_select(0)
    assert np.array_equal(_u32(reg.scan_download(0)), _u32(frame))
    # ... also by lii_scan_sort, which sorts it from where the ingest left it
    reg.frame_select(0)
    reg.scan_sort()
    assert np.array_equal(_u32(reg.scan_download(0)), _u32(oracle.sort_by_time(frame)))
    reg.frame_select(0)
    assert np.array_equal(_u32(reg.scan_download(0)), _u32(frame))
    reg.close()


# ------------------------------------------------------------------------------------------------ 5. read-only source, pre-arm
def test_sort_job_reads_scan_dev_only_and_arms_nothing(oracle):
    import lidar_imu_init_amd as lii
    _, map_pts, scan, _, _, _ = _world()
    fresh_sort = _cache.get("poses_sorted2") or _register("poses", scan, 2)
    sorted_scan = oracle.sort_by_time(scan)
    fresh_plain = _register("poses", sorted_scan, 1, scan_dev=True)
    reg = _registrar(len(map_pts))
    reg.map_build(map_pts)
    # (_register uploads `scan` into a device buffer of its own, adopts it with scan_sorted = 2 and names it as the next scan as well)
    a = _register("poses", scan, 2, scan_dev=True, next_scan=True, reg=reg)
    _same(a, fresh_sort, "a sort job that names next_scan_dev")
    reg.scan_set_device(a["dev"])  # (the caller's buffer, read back through the handle)
    assert np.array_equal(_u32(reg.scan_download(0)), _u32(scan)), "the caller's scan_dev buffer must hold its original bytes"
    # nothing waits on the stream, and the next scan_sorted = 1 job is what it is on a fresh handle
    import time
    t0 = time.perf_counter()
    reg.synchronize()
    assert time.perf_counter() - t0 < 0.5  # (a launch left waiting would hold the stream for 2 s)
    b = _register("poses", sorted_scan, 1, scan_dev=True, reg=reg)
    _same(b, fresh_plain, "the scan_sorted = 1 job behind a sort job")
    reg.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_scan_sort_refusals_and_the_abi5_job(oracle):
    import lidar_imu_init_amd as lii
    from lidar_imu_init_amd import api
    _, map_pts, scan, _, _, st0 = _world()
    reg = _registrar(len(map_pts))
    assert reg.L.lii_scan_sort(None) == -1
    with pytest.raises(lii.LIIError) as e:
        reg.scan_sort()
    assert e.value.code == -5  # LII_ERR_STATE: no scan
    reg.map_build(map_pts)
    s0 = lii.State(st0)
    T = _pose_table(s0)

    def abi5(scan_sorted):
        reg.scan_upload(scan)
        job = api.lii_scan_job()
        job.struct_size, job.undistort, job.leaf = 48, 1, LEAF
        job.imu_poses, job.n_imu_poses = T.ctypes.data, len(T)
        job.opts = api.lii_iekf_opts(MAX_IT, 0)
        job.scan_sorted = scan_sorted  # (the padding word at the end of the 48-byte job of ABI 5: not a field of that job)
        st, rep = s0.copy(), api.lii_iekf_report()
        assert reg.L.lii_scan_register(reg.h, C.byref(job), st.pod.ctypes.data, s0.pod.ctypes.data, C.byref(rep)) == 0
        return _results(reg, st, dict(iterations=rep.iterations, searches=rep.searches, effect_num=rep.effect_num))

    a, b = abi5(0), abi5(2)
    _same(a, b, "a job of struct_size 48 with 2 in the word behind it")
    assert np.array_equal(a["scan"][:, 3], scan[:, 3])  # (input order: nothing was sorted)
    # a communicator attached: single rank only for now
    reg.scan_upload(scan)
    reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")
    with pytest.raises(lii.LIIError) as e:
        reg.scan_sort()
    assert e.value.code == -5
    with pytest.raises(lii.LIIError) as e:
        reg.scan_register(s0.copy(), s0, imu_poses=T, leaf=LEAF, max_iterations=MAX_IT, scan_sorted=2)
    assert e.value.code == -5
    reg.comm_destroy()
    assert np.array_equal(_u32(reg.scan_download(0)), _u32(scan))  # (the refused calls left the scan alone)
    reg.close()


# ------------------------------------------------------------------------------------------------ 7. lazy allocation
def test_sort_buffers_come_with_the_first_sort_and_go_with_the_handle(oracle):
    """The sort's buffers (keys, indices, the gather target: 32 bytes per point of max_scan_points, + the radix sort's temporary storage)
    are the only device memory this feature adds to a handle.  Read as tests/test_gpu_handle_lifecycle.py reads it (hipMemGetInfo): a
    handle that registers scan_sorted = 0 / 1 scans holds the same memory before and after them - none of the buffers; its first sort
    adds at least the 32 bytes per point - so they were not there before; close() returns everything (bound: one scan buffer, as there)."""
    import torch

    import lidar_imu_init_amd as lii
    _, map_pts, scan, _, _, st0 = _world()
    MAX_SCAN = 400_000
    s0 = lii.State(st0)
    T = _pose_table(s0)

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free

    def job(reg, scan_sorted):
        reg.scan_upload(scan if scan_sorted != 1 else oracle.sort_by_time(scan))
        reg.scan_register(s0.copy(), s0, imu_poses=T, leaf=LEAF, max_iterations=MAX_IT, scan_sorted=scan_sorted)
        reg.synchronize()

    log = []
    for cycle in range(2):  # (the first one is the warm-up: the runtime's own pools)
        before = used()
        reg = _registrar(len(map_pts), max_scan_points=MAX_SCAN)
        reg.map_build(map_pts)
        job(reg, 0)
        job(reg, 1)
        plain0 = used()
        job(reg, 0)
        job(reg, 1)
        plain1 = used()
        job(reg, 2)
        sorting = used()
        job(reg, 2)
        reg.scan_sort()
        sorting2 = used()
        reg.close()
        after = used()
        log.append((before, plain0, plain1, sorting, sorting2, after))
        print(f"cycle {cycle}: handle with 0 / 1 jobs {plain0 - before} bytes, after more of them {plain1 - plain0:+d}, first sort "
              f"{sorting - plain1:+d}, more sorts {sorting2 - sorting:+d}, after close {after - before:+d}")
    before, plain0, plain1, sorting, sorting2, after = log[1]
    bound = 16 * MAX_SCAN  # (one scan buffer: what a neighbour on the device may move the reading by, as in the lifecycle test)
    assert abs(plain1 - plain0) <= bound
    assert sorting - plain1 >= 32 * MAX_SCAN
    assert abs(sorting2 - sorting) <= bound
    assert after - before <= bound
