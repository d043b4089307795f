"""The optional intensity channel (lii_scan_intensity_*, lii_ingest_set_intensity, LII_PUB_INTENSITY): one float per point beside the
float4 clouds, carried by every stage that reorders, drops, merges or republishes points.

Expected values never come from the library:
  ingest   the frames are the oracle's (oracle.ingest_pcl2 / ingest_livox: x, y, z, t); a frame point's intensity is looked up by the bit
           pattern of its (x, y, z) in the message the test built - the ingest copies x, y, z unchanged and the test asserts that the
           triples of its message are pairwise distinct;
  sort     intensity[np.argsort(t with -0.0 as +0.0, kind="stable")];
  voxels   column 3 of oracle.voxel_grid(np.c_[xyz, intensity], leaf): the oracle sums its fourth column exactly as PCL sums every field
           (oracle/orc_scan.hpp:130-143), in the order lii_scan_download(h, 1) returns the points (ascending PCL voxel index).  No voxel of
           a test cloud holds more than 512 points (asserted with numpy): beyond that the hashed emit is right to rounding only;
  publish  the above, matched to the published rows.
Every comparison is bit for bit (uint32 views).  Scans hold at most 5 000 points, the map a few thousand."""
import ctypes as C
import os

import numpy as np
import pytest

from harness import synth, wire

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, STATE = -1, -4, -5
DENSE, DOWN, EFFECT, BODY, INTENSITY = 1, 2, 4, 8, 16
MAX_SCAN = 8192
_cache = {}


# ------------------------------------------------------------------------------------------------ helpers
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _code(fn):
    import lidar_imu_init_amd as lii
    try:
        fn()
    except lii.LIIError as e:
        return e.code
    return 0


def _with_env(make, **env):
    """make() under the given environment switches (the library reads them when a handle is created), restored afterwards"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return make()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _plain(**env):
    import lidar_imu_init_amd as lii
    return _with_env(lambda: lii.Registrar(max_scan_points=MAX_SCAN, max_map_points=1000, filter_size_map=0.2), **env)


def _floats(n, seed):
    """n distinct positive floats with non-trivial mantissas"""
    rng = np.random.default_rng(seed)
    v = (rng.uniform(0.5, 255.0, n) * (1.0 + rng.uniform(0, 1e-3, n))).astype(np.float32)
    assert len(np.unique(_bits(v))) > 0.99 * n
    return v


# ------------------------------------------------------------------------------------------------ ingest
def _message_xyz(n, seed):
    """n points: most in a shell of 2 .. 20 m, every ninth inside the blind zone (< 1 m), every eleventh NaN; all triples distinct"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    r = rng.uniform(2.0, 20.0, n)
    k = np.arange(n)
    r[k % 9 == 4] = rng.uniform(0.1, 0.8, int((k % 9 == 4).sum()))
    xyz = (d * r[:, None]).astype(np.float32)
    nan = (k % 11 == 7)
    return xyz, nan


def _lookup(xyz, inten):
    keys = [xyz[i].tobytes() for i in range(len(xyz))]
    assert len(set(keys)) == len(keys), "the test's message must hold pairwise distinct (x, y, z) triples"
    fin = np.isfinite(xyz).all(1)
    fk = [keys[i] for i in np.nonzero(fin)[0]]
    assert len(set(fk)) == len(fk)
    return dict(zip(keys, np.asarray(inten, np.float32)))


def _pcl2_message(lidar_type, n, seed, ordered=True):
    """(bytes, lookup (x, y, z) bits -> expected float intensity).  ordered: time stamps ascending in input order; else a shuffled sweep."""
    xyz, nan = _message_xyz(n, seed)
    xyz[nan] = np.nan
    xyz[nan, 1] = np.arange(n, dtype=np.float32)[nan]  # (NaN points keep distinct bit patterns: x = NaN, y = their index)
    rng = np.random.default_rng(seed + 1)
    t_ms = np.linspace(1.0, 99.0, n) if n > 1 else np.array([50.0])  # (all positive: the message carries per-point time, nothing is synthesised)
    if not ordered:
        t_ms = rng.permutation(t_ms)
    ring = rng.integers(0, 18, n).astype(np.int32)  # rings 16 and 17 are beyond N_SCANS = 16
    raw = wire.pack_pcl2(lidar_type, xyz, ring, t_ms, 1000.0)
    a = np.frombuffer(raw, wire.DTYPES[lidar_type]).copy()
    if lidar_type == wire.L515:
        return a.tobytes(), _lookup(xyz, np.zeros(n, np.float32))
    if lidar_type == wire.ROBOSENSE:
        val = rng.permutation(np.arange(n) % 256).astype(np.uint8)  # 0 ... 255, all of them once n >= 256
    else:
        val = _floats(n, seed + 2)
    a["intensity"] = val
    return a.tobytes(), _lookup(xyz, val.astype(np.float32))


def _livox_message(n, seed, ordered=True):
    xyz, _ = _message_xyz(n, seed)  # (blind-zone points, no NaN: the CustomMsg path has no NaN test and its drivers publish none)
    rng = np.random.default_rng(seed + 1)
    a = np.zeros(n, wire.LIVOX_DTYPE)
    a["x"], a["y"], a["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    t = np.linspace(0.0, 99.0, n) if n > 1 else np.array([50.0])
    if not ordered:
        t = rng.permutation(t)
    a["offset_time"] = np.round(t * 1e6).astype(np.uint32)
    val = rng.permutation(np.arange(n) % 256).astype(np.uint8)
    a["reflectivity"] = val
    a["line"] = rng.integers(0, 7, n)  # line 6 is beyond N_SCANS = 6
    tag = np.where(rng.random(n) < 0.9, 0x10, 0x00).astype(np.uint8)
    tag[rng.random(n) < 0.05] = 0x20
    a["tag"] = tag
    return a.tobytes(), _lookup(xyz, val.astype(np.float32))


def _ingest_both(reg, oracle, lidar_type, raw, n, cut, begin=False):
    """(device frame table, oracle frames) of one message; begin: put under way only (the caller ends it)"""
    stamp = 1000.0
    if lidar_type == wire.AVIA:
        f = wire.livox_fields()
        orc = oracle.ingest_livox(raw, n, f, 6, 1, 1.0, stamp, cut, 100)
        orc = [fr for fr in orc if cut != 0 or len(fr[1])]  # (a whole message that leaves no point yields no frame: the node skips an empty cloud)
        if begin:
            return reg.ingest_livox_begin(raw, n, f, 6, 1, 1.0, stamp, cut, 100), orc
        return reg.ingest_livox(raw, n, f, 6, 1, 1.0, stamp, cut, 100), orc
    f = wire.pc2_fields(lidar_type)
    orc = [fr for fr in oracle.ingest_pcl2(raw, n, f, lidar_type, 16, 1, 1.0, stamp, cut, 100) if cut != 0 or len(fr[1])]
    if begin:
        return reg.ingest_pcl2_begin(raw, n, f, lidar_type, 16, 1, 1.0, stamp, cut, 100), orc
    return reg.ingest_pcl2(raw, n, f, lidar_type, 16, 1, 1.0, stamp, cut, 100), orc


def _check_frames(reg, info, orc, lut, what):
    assert len(info) == len(orc), what
    total = 0
    for k, (tb, pts_o) in enumerate(orc):
        reg.frame_select(k)
        exp = np.array([lut[pts_o[i, :3].tobytes()] for i in range(len(pts_o))], np.float32)
        got = reg.scan_intensity_download(0)  # (asked for first: the frame still lies where the ingest left it)
        pts = reg.scan_download(0)
        again = reg.scan_intensity_download(0)  # (... and once more, after the frame has moved into the handle's own buffer)
        assert np.array_equal(_bits(pts), _bits(pts_o)), f"{what}: frame {k} differs from the oracle's"
        assert got.shape == exp.shape and np.array_equal(_bits(got), _bits(exp)), f"{what}: intensities of frame {k}: {int((_bits(got) != _bits(exp)).sum())} differ"
        assert np.array_equal(_bits(again), _bits(exp))
        total += len(pts_o)
    return total


@pytest.fixture(scope="module")
def ingest_reg():
    r = _plain()
    r.ingest_set_intensity(True)
    yield r
    r.close()


INGEST_CASES = [(wire.VELO, 1), (wire.VELO, 3), (wire.VELO, 0), (wire.OUSTER, 1), (wire.OUSTER, 3), (wire.OUSTER, 0), (wire.PANDAR, 1),
                (wire.PANDAR, 3), (wire.ROBOSENSE, 1), (wire.ROBOSENSE, 3), (wire.AVIA, 1), (wire.AVIA, 3), (wire.AVIA, 0)]


@pytest.mark.parametrize("lidar_type,cut", INGEST_CASES)
def test_ingest_frames_carry_the_message_intensity(ingest_reg, oracle, lidar_type, cut):
    seen = 0
    for n in (1, 2, 255, 257, 3000):
        for ordered in (True, False):
            raw, lut = (_livox_message if lidar_type == wire.AVIA else _pcl2_message)(*([n, 10 * n + cut, ordered] if lidar_type == wire.AVIA else [lidar_type, n, 10 * n + cut, ordered]))
            info, orc = _ingest_both(ingest_reg, oracle, lidar_type, raw, n, cut)
            seen += _check_frames(ingest_reg, info, orc, lut, f"type {lidar_type} cut {cut} n {n} ordered {ordered}")
    print(f"type {lidar_type} cut {cut}: {seen} frame points compared")
    assert seen > 3000


def test_ingest_redo_delivers_the_redone_frames_intensity(oracle):
    """A time-ordered message, then an unordered one: the second is enqueued without its time sort (the first one's prediction), fails the
    order check on the device and is cut again behind the sort (ingest_redo_sorted) - the intensities are those of the redone frames."""
    reg = _plain()
    reg.ingest_set_intensity(True)
    for lidar_type in (wire.OUSTER, wire.AVIA):
        make = (lambda n, s, o: _livox_message(n, s, o)) if lidar_type == wire.AVIA else (lambda n, s, o: _pcl2_message(lidar_type, n, s, o))
        raw, lut = make(3000, 5, True)
        info, orc = _ingest_both(reg, oracle, lidar_type, raw, 3000, 3)
        assert _check_frames(reg, info, orc, lut, "ordered message") > 1500
        raw, lut = make(3000, 6, False)
        info, orc = _ingest_both(reg, oracle, lidar_type, raw, 3000, 3)
        assert _check_frames(reg, info, orc, lut, "unordered message behind an ordered one") > 1500
        # (and the ordered one again behind it: sorted this time, since the last message was not in order)
        raw, lut = make(2000, 7, True)
        info, orc = _ingest_both(reg, oracle, lidar_type, raw, 2000, 3)
        assert _check_frames(reg, info, orc, lut, "ordered message behind an unordered one") > 1000
    reg.close()


def test_ingest_overlapped_two_messages_under_way(oracle):
    reg = _plain()
    reg.ingest_set_intensity(True)
    for lidar_type in (wire.VELO, wire.AVIA):
        make = (lambda n, s, o: _livox_message(n, s, o)) if lidar_type == wire.AVIA else (lambda n, s, o: _pcl2_message(lidar_type, n, s, o))
        msgs = [make(3000, 21, True), make(2500, 22, False), make(257, 23, True)]
        orcs = []
        for raw, _ in msgs[:2]:
            orcs.append(_ingest_both(reg, oracle, lidar_type, raw, len(raw) // (20 if lidar_type == wire.AVIA else 32), 3, begin=True)[1])
        for m in range(3):
            info = reg.ingest_end()
            # the frames of message m are checked while message m + 1 (and, put under way now, m + 2) is under way
            if m == 0:
                raw2 = msgs[2][0]
                orcs.append(_ingest_both(reg, oracle, lidar_type, raw2, len(raw2) // (20 if lidar_type == wire.AVIA else 32), 3, begin=True)[1])
            assert _check_frames(reg, info, orcs[m], msgs[m][1], f"type {lidar_type} overlapped message {m}") > 100
    reg.close()


def test_ingest_l515_yields_zeros_and_order_off_yields_none(oracle):
    reg = _plain()
    raw, lut = _pcl2_message(wire.OUSTER, 3000, 31, True)
    # the order off: no intensities, and the frames are what they were
    info, orc = _ingest_both(reg, oracle, wire.OUSTER, raw, 3000, 3)
    for k, (_, pts_o) in enumerate(orc):
        reg.frame_select(k)
        assert _code(lambda: reg.scan_intensity_download(0)) == STATE
        assert np.array_equal(_bits(reg.scan_download(0)), _bits(pts_o))
        assert _code(lambda: reg.scan_intensity_download(0)) == STATE
    reg.ingest_set_intensity(True)
    info, orc = _ingest_both(reg, oracle, wire.OUSTER, raw, 3000, 3)
    assert _check_frames(reg, info, orc, lut, "order on") > 1500
    # an L515 message (one frame whatever the cut): zeros
    rawl, lutl = _pcl2_message(wire.L515, 3000, 32, True)
    f = wire.pc2_fields(wire.L515)
    info = reg.ingest_pcl2(rawl, 3000, f, wire.L515, 16, 1, 1.0, 1000.0, 0, 100)
    orc = oracle.ingest_pcl2(rawl, 3000, f, wire.L515, 16, 1, 1.0, 1000.0, 0, 100)
    assert len(info) == 1
    reg.frame_select(0)
    got = reg.scan_intensity_download(0)
    assert len(got) == len(orc[0][1]) > 2000 and not _bits(got).any()
    # the order taken back: a frame ingested without it detaches what the scan before had
    reg.ingest_set_intensity(False)
    info, orc = _ingest_both(reg, oracle, wire.OUSTER, raw, 3000, 1)
    reg.frame_select(0)
    assert _code(lambda: reg.scan_intensity_download(0)) == STATE
    reg.close()


# ------------------------------------------------------------------------------------------------ time sort
def _stamps(n, seed):
    """time stamps with ties, -0.0 / +0.0 and a descending run"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, 100.0, n).astype(np.float32)
    if n >= 2:
        t[0], t[1] = 0.0, -0.0
    if n > 16:
        t[n // 2:n // 2 + n // 4] = np.linspace(90.0, 10.0, n // 4, dtype=np.float32)  # a descending run
        t[3::5] = t[2::5][:len(t[3::5])]  # ties: every fifth stamp repeats the one before it
        t[5], t[n - 1] = -0.0, 0.0
        assert (np.diff(t) == 0).sum() >= n // 6 and (np.diff(t) < 0).sum() >= n // 8
    return t


def _sort_perm(t):
    key = np.where(t == 0, np.float32(0.0), t)  # (-0.0 as +0.0)
    return np.argsort(key, kind="stable")


@pytest.mark.parametrize("n", [1, 2, 257, 5000])
def test_scan_sort_moves_the_intensity(n):
    rng = np.random.default_rng(n)
    scan = np.c_[rng.normal(size=(n, 3)) * 5, _stamps(n, n)].astype(np.float32)
    inten = _floats(n, n + 1)
    perm = _sort_perm(scan[:, 3])
    reg = _plain()
    for via in ("upload", "device"):
        if via == "upload":
            reg.scan_upload(scan)
            reg.scan_intensity_upload(inten)
        else:
            reg.scan_set_device(reg.device_scan(scan))
            reg.scan_intensity_set_device(reg.device_intensity(inten))
        assert np.array_equal(_bits(reg.scan_intensity_download(0)), _bits(inten))
        reg.scan_sort()
        assert np.array_equal(_bits(reg.scan_download(0)), _bits(scan[perm]))
        got = reg.scan_intensity_download(0)
        assert np.array_equal(_bits(got), _bits(inten[perm])), f"n {n} via {via}: {int((_bits(got) != _bits(inten[perm])).sum())} differ"
    # the PointXYZINormal layout: stride 48, intensity at 32
    rec = np.zeros((n, 12), np.float32)
    rec[:, :3], rec[:, 8], rec[:, 9] = scan[:, :3], inten, scan[:, 3]
    reg.scan_upload(rec)
    reg.scan_intensity_upload(rec)
    assert np.array_equal(_bits(reg.scan_intensity_download(0)), _bits(inten))
    reg.close()


# ------------------------------------------------------------------------------------------------ a small world for the registrations
def _world():
    """hall, map points (a few thousand), true pose, a 16 384-ray scan from it, a start state a little off (tests/test_gpu_publish.py's)"""
    if "w" not in _cache:
        import lidar_imu_init_amd as lii
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
        assert len(map_pts) <= 20_000
        _cache["w"] = dict(hall=hall, map=map_pts, R=R, p=p, scan=scan, st=st)
    return _cache["w"]


def _registrar(**env):
    import lidar_imu_init_amd as lii
    w = _world()
    reg = _with_env(lambda: lii.Registrar(max_scan_points=MAX_SCAN, max_map_points=50_000, filter_size_map=0.15), **env)
    reg.map_build(w["map"])
    return reg


def _to_world(state, pts4):
    """pointBodyToWorld by the oracle at `state`, the fourth column carried through"""
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


def _poses():
    P = np.zeros((3, 22))
    for k, t in enumerate((0.0, 0.05, 0.1)):
        P[k, 0] = t
        P[k, 1:4] = [0.1, -0.05, 0.02]
        P[k, 4:7] = [0.02, -0.01, 0.05]
        P[k, 7:10] = [0.3, -0.2, 0.05]
        P[k, 10:13] = np.array([0.3, -0.2, 0.05]) * t
        P[k, 13:22] = synth.rot_zyx(0.02 * t, -0.01 * t, 0.05 * t).reshape(-1)
    return P


def _imu_rows(t_beg):
    t = t_beg + np.arange(0, 11) * 0.01
    rows = np.zeros((len(t), 7))
    rows[:, 0] = t
    rows[:, 1:4] = [0.01, -0.02, 0.03]
    rows[:, 4:7] = [0.05, -0.03, 9.81]
    return rows


def _take(n, sorted_):
    s = _world()["scan"]
    idx = np.linspace(0, len(s) - 1, n).astype(int) if n > 1 else np.array([len(s) // 2])
    s = s[idx]
    return s[np.argsort(s[:, 3], kind="stable")] if sorted_ else s


def _register(reg, form, st, **kw):
    """one registration in the given form; returns the report"""
    if form == "poses":
        return reg.scan_register(st, st.copy(), imu_poses=_poses(), **kw)
    if form == "cv":
        return reg.register_cv(0.1, 1.0, 1.0, st, **kw)[2]
    assert form == "imu"
    reg.set_imu_noise(cov_gyr=0.1, cov_acc=0.1, mean_acc_norm=9.81)
    reg.imu_carry = dict(last_imu=np.r_[99.99, 0.01, -0.02, 0.03, 0.05, -0.03, 9.81], last_lidar_end_time=99.995)
    return reg.register_imu(_imu_rows(100.0), 100.0, st, imu_en=True, **kw)[2]


def _state(form):
    st = _world()["st"].copy()
    if form == "cv":
        st.bias_g[:] = [0.01, -0.02, 0.03]
        st.vel_end[:] = [0.3, -0.2, 0.05]
    return st


@pytest.mark.parametrize("n", [1, 2, 257, 5000])
@pytest.mark.parametrize("form", ["poses", "imu", "cv"])
def test_a_job_that_sorts_publishes_the_sorted_intensity(form, n):
    """scan_sorted = 2 inside lii_scan_register / _imu / _cv: read back from the BODY (and DENSE) publish intensity"""
    scan = _take(n, False).copy()
    scan[:, 3] = _stamps(n, 7 * n)
    inten = _floats(n, n + 3)
    perm = _sort_perm(scan[:, 3])
    reg = _registrar()
    reg.publish_set(BODY | DENSE | INTENSITY, to_host=True)
    reg.scan_upload(scan)
    reg.scan_intensity_upload(inten)
    _register(reg, form, _state(form), leaf=0.2, max_iterations=3, scan_sorted=2)
    body = reg.publish_fetch(BODY)
    assert np.array_equal(_bits(body[:, 3]), _bits(scan[perm, 3]))
    for cloud in (BODY, DENSE):
        got = reg.publish_fetch_intensity(cloud)
        assert got.shape == (n,) and np.array_equal(_bits(got), _bits(inten[perm])), f"{form} n {n} cloud {cloud}"
    assert np.array_equal(_bits(reg.scan_intensity_download(0)), _bits(inten[perm]))
    reg.close()


# ------------------------------------------------------------------------------------------------ voxel filter
def _voxel_cloud(kind, seed=11, leaf=0.5):
    """A cloud whose voxels at `leaf` hold prescribed numbers of points, shuffled (the members of a voxel are spread over the input):
    sparse: 1 ... 10 per voxel (the members a slot of the hashed table holds itself); crowded: also 11 ... 40 (the list behind them) and a
    few voxels of a few hundred."""
    rng = np.random.default_rng(seed)
    counts = list(rng.integers(1, 3, 700)) + list(range(2, 11)) * 12
    if kind == "crowded":
        counts += list(range(11, 41)) * 2 + [150, 260, 400]
    pts = []
    cells = rng.permutation(40 * 40 * 6)[:len(counts)]
    for c, k in zip(cells, counts):
        org = np.array([c % 40 - 20, (c // 40) % 40 - 20, c // 1600 - 3], np.float64) * leaf
        pts.append(org + rng.uniform(0.05, 0.95, (int(k), 3)) * leaf)
    xyz = np.concatenate(pts).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    assert len(xyz) <= 5000
    scan = np.c_[xyz, np.sort(rng.uniform(0, 100, len(xyz)))].astype(np.float32)
    return scan, _floats(len(scan), seed + 1)


def _max_per_voxel(xyz, leaf):
    inv = np.float32(1.0) / np.float32(leaf)
    v = np.floor(xyz[:, :3].astype(np.float32) * inv).astype(np.int64)
    _, cnt = np.unique(v, axis=0, return_counts=True)
    return int(cnt.max()), cnt


def _expect_voxels(oracle, xyz, inten, leaf):
    mx, _ = _max_per_voxel(xyz, leaf)
    assert mx <= 512, "a condition on the test's cloud: beyond 512 points per voxel the hashed emit is right to rounding only"
    exp, _ = oracle.voxel_grid(np.c_[xyz[:, :3], inten].astype(np.float32), leaf)
    return exp


VOXEL_PATHS = [("hash", "crowded", dict(LII_VOXEL_FILTER="hash")), ("sort", "crowded", dict(LII_VOXEL_FILTER="sort")),
               ("auto", "sparse", {}), ("auto", "crowded", {}), ("emit_late", "crowded", dict(LII_VOXEL_FILTER="hash", LII_TEST="emit_late")),
               ("emit_late", "sparse", dict(LII_TEST="emit_late"))]


@pytest.mark.parametrize("path,kind,env", VOXEL_PATHS)
def test_voxel_filter_forms_pcl_centroid_of_intensity(oracle, path, kind, env):
    leaf = 0.5
    scan, inten = _voxel_cloud(kind)
    mx, cnt = _max_per_voxel(scan, leaf)
    assert (cnt == 1).any() and ((cnt >= 2) & (cnt <= 10)).any()
    if kind == "crowded":
        assert ((cnt >= 11) & (cnt <= 40)).any() and (cnt > 100).sum() >= 3 and mx <= 512
    exp = _expect_voxels(oracle, scan, inten, leaf)
    exp_t, _ = oracle.voxel_grid(scan, leaf)
    reg = _plain(**env)
    reg.scan_upload(scan)
    n0, _ = reg.downsample(leaf)
    plain = reg.scan_download(1)
    assert _code(lambda: reg.scan_intensity_download(1)) == STATE
    for rep in range(2):  # (the second run of a leaf is not probed any more)
        reg.scan_upload(scan)
        reg.scan_intensity_upload(inten)
        n1, filt = reg.downsample(leaf)
        down = reg.scan_download(1)
        got = reg.scan_intensity_download(1)
        print(f"{path} / {kind}: {len(scan)} points -> {n1} voxels, largest {mx}")
        assert n1 == n0 == len(exp) and filt
        assert np.array_equal(_bits(down), _bits(plain)) and np.array_equal(_bits(down), _bits(exp_t))  # the same xyzt with and without
        assert np.array_equal(_bits(down[:, :3]), _bits(exp[:, :3]))
        bad = int((_bits(got) != _bits(exp[:, 3])).sum())
        assert bad == 0, f"{path} / {kind}: {bad} of {len(got)} voxel intensities differ from PCL's centroid"
    reg.close()


def test_voxel_filter_pass_through_forms(oracle):
    """PCL's overflow guard (dx dy dz > INT32_MAX: the cloud passes unfiltered) on both filters, and lii_downsample_skip: a copy"""
    scan, inten = _voxel_cloud("sparse", seed=13)
    leaf = 0.004  # 20 m / 0.004 = 5 000 cells per axis, x 750 in z: more than 2^31 voxels
    for env in ({}, dict(LII_VOXEL_FILTER="sort"), dict(LII_VOXEL_FILTER="hash")):
        reg = _plain(**env)
        reg.scan_upload(scan)
        reg.scan_intensity_upload(inten)
        n1, filt = reg.downsample(leaf)
        exp, filt_o = oracle.voxel_grid(np.c_[scan[:, :3], inten].astype(np.float32), leaf)
        assert not filt and not filt_o and n1 == len(scan) == len(exp)
        assert np.array_equal(_bits(reg.scan_download(1)), _bits(scan))
        assert np.array_equal(_bits(reg.scan_intensity_download(1)), _bits(exp[:, 3]))
        assert np.array_equal(_bits(exp[:, 3]), _bits(inten))
        assert reg.downsample_skip() == len(scan)
        assert np.array_equal(_bits(reg.scan_intensity_download(1)), _bits(inten))
        reg.scan_upload(scan)  # (replaces the scan: nothing attached any more)
        reg.downsample_skip()
        assert _code(lambda: reg.scan_intensity_download(1)) == STATE and _code(lambda: reg.scan_intensity_download(0)) == STATE
        reg.close()


FUSED = [("poses", True, dict(LII_VOXEL_FILTER="hash")), ("poses", False, dict(LII_VOXEL_FILTER="hash")), ("cv", True, dict(LII_VOXEL_FILTER="hash")),
         ("imu", True, dict(LII_VOXEL_FILTER="hash")), ("poses", True, {}), ("cv", True, {}), ("imu", True, {}), ("poses", True, dict(LII_TEST="no_fuse"))]


@pytest.mark.parametrize("form,sorted_,env", FUSED)
def test_voxel_filter_inside_a_registration(oracle, form, sorted_, env):
    """The filter behind a de-skew (its insert fused into the de-skew launch once the leaf is known to be sparse - at once under
    LII_VOXEL_FILTER=hash): xyz are de-skewed first, so the expectation is formed from lii_scan_download(h, 0) after the call."""
    leaf = 0.5
    scan = _take(5000, sorted_)
    inten = _floats(len(scan), 41)
    reg = _registrar(**env)
    for rep in range(2):  # (second scan of the leaf: fused on a handle that probes)
        reg.scan_upload(scan)
        reg.scan_intensity_upload(inten)
        _register(reg, form, _state(form), leaf=leaf, max_iterations=3, scan_sorted=sorted_)
        desk = reg.scan_download(0)
        assert np.array_equal(_bits(desk[:, 3]), _bits(scan[:, 3])) and not np.array_equal(_bits(desk[:, :3]), _bits(scan[:, :3]))
        exp = _expect_voxels(oracle, desk, inten, leaf)
        down, got = reg.scan_download(1), reg.scan_intensity_download(1)
        assert len(exp) == len(down) < len(scan) and _max_per_voxel(desk, leaf)[0] >= 3 and np.array_equal(_bits(down[:, :3]), _bits(exp[:, :3]))
        bad = int((_bits(got) != _bits(exp[:, 3])).sum())
        assert bad == 0, f"{form} sorted {sorted_} {env} scan {rep}: {bad} of {len(got)} differ"
    # ... and the same down-sampled xyzt without intensities attached
    reg.scan_upload(scan)
    _register(reg, form, _state(form), leaf=leaf, max_iterations=3, scan_sorted=sorted_)
    assert np.array_equal(_bits(reg.scan_download(1)), _bits(down))
    assert _code(lambda: reg.scan_intensity_download(1)) == STATE
    reg.close()


# ------------------------------------------------------------------------------------------------ publish
def _fetch(reg, cloud, to_host, intensity=False):
    """One published cloud (or its intensities).  to_host: the library's pinned copy.  Otherwise the DEVICE buffer the fetch hands out,
    read back through a second handle (lii_scan_set_device / lii_scan_intensity_set_device copy from any device pointer, the
    downloads return what they copied): nothing but the library under test touches the device in this process."""
    if to_host:
        return reg.publish_fetch_intensity(cloud) if intensity else reg.publish_fetch(cloud)
    hp, dp, n = C.c_void_p(), C.c_void_p(), C.c_int32(0)
    fn = reg.L.lii_publish_fetch_intensity if intensity else reg.L.lii_publish_fetch
    reg._check(fn(reg.h, int(cloud), C.byref(hp), C.byref(dp), C.byref(n)))
    assert not hp.value and dp.value  # (no host copy was ordered)
    if n.value == 0:
        return np.zeros(0 if intensity else (0, 4), np.float32)
    if "reader" not in _cache:
        _cache["reader"] = _plain()
    rd = _cache["reader"]
    if intensity:
        rd.scan_upload(np.zeros((n.value, 4), np.float32))
        rd.scan_intensity_set_device((dp, n.value))
        return rd.scan_intensity_download(0)
    rd.scan_set_device((dp, n.value))
    return rd.scan_download(0)


@pytest.mark.parametrize("to_host", [True, False])
@pytest.mark.parametrize("sort_first", [False, True])
def test_published_intensities(oracle, to_host, sort_first):
    leaf = 0.25
    scan = _take(4099, not sort_first)
    inten = _floats(len(scan), 51)
    perm = _sort_perm(scan[:, 3]) if sort_first else np.arange(len(scan))
    reg = _registrar()
    reg.publish_set(DENSE | DOWN | EFFECT | BODY | INTENSITY, to_host=to_host)
    st = _state("poses")
    reg.scan_upload(scan)
    reg.scan_intensity_upload(inten)
    _register(reg, "poses", st, leaf=leaf, max_iterations=4, scan_sorted=2 if sort_first else True)
    dense, body, down = _fetch(reg, DENSE, to_host), _fetch(reg, BODY, to_host), _fetch(reg, DOWN, to_host)
    assert np.array_equal(_bits(dense[:, 3]), _bits(scan[perm, 3]))
    for cloud in (DENSE, BODY):
        got = _fetch(reg, cloud, to_host, intensity=True)
        assert np.array_equal(_bits(got), _bits(inten[perm])), cloud
    # DOWN: row by row with the DOWN cloud (the device's order) - the oracle's centroids of the de-skewed scan, taken to the world
    exp_i = _expect_voxels(oracle, body, inten[perm], leaf)
    cen, _ = oracle.voxel_grid(body, leaf)
    assert np.array_equal(_bits(cen[:, :3]), _bits(exp_i[:, :3]))
    ref = _to_world(st, cen)
    at = {r.tobytes(): i for i, r in enumerate(_bits(ref))}
    assert len(at) == len(ref) == len(down)
    rows = np.array([at[r.tobytes()] for r in _bits(down)])
    got = _fetch(reg, DOWN, to_host, intensity=True)
    assert got.shape == (len(down),)
    bad = int((_bits(got) != _bits(exp_i[rows, 3])).sum())
    assert bad == 0, f"{bad} of {len(got)} DOWN intensities differ"
    assert _code(lambda: reg.publish_fetch_intensity(EFFECT)) == INVALID
    # lii_publish_now serves the same from the handle's current clouds
    reg.publish_now(st)
    assert np.array_equal(_bits(_fetch(reg, DOWN, to_host, intensity=True)), _bits(got))
    assert np.array_equal(_bits(_fetch(reg, DENSE, to_host, intensity=True)), _bits(inten[perm]))
    reg.close()


def test_fetch_from_while_waiting_and_two_deep_lifetime():
    reg = _registrar()
    reg.publish_set(DENSE | BODY | INTENSITY, to_host=True)
    scans = [_take(n, True) for n in (3000, 2500, 2000)]
    intens = [_floats(len(s), 60 + k) for k, s in enumerate(scans)]
    seen = {}

    def hook(m):
        # scan m - 1's intensities are fetched while scan m is registered: views of the library's pinned buffers
        seen[m - 1] = (reg.publish_fetch_intensity(DENSE, copy=False), reg.publish_fetch_intensity(BODY, copy=False), reg.publish_fetch(DENSE, copy=False))
        assert np.array_equal(_bits(seen[m - 1][0]), _bits(intens[m - 1]))

    st = _state("poses")
    for m, (s, it) in enumerate(zip(scans, intens)):
        reg.scan_upload(s)
        reg.scan_intensity_upload(it)
        _register(reg, "poses", st, leaf=0.2, max_iterations=3, scan_sorted=True, while_waiting=(lambda m=m: hook(m)) if m > 0 else None)
        if m > 0:  # scan m - 1's are intact after scan m has run (two deep) ...
            assert np.array_equal(_bits(seen[m - 1][0]), _bits(intens[m - 1])) and np.array_equal(_bits(seen[m - 1][1]), _bits(intens[m - 1]))
            assert len(seen[m - 1][2]) == len(scans[m - 1])
        assert np.array_equal(_bits(reg.publish_fetch_intensity(DENSE)), _bits(it))  # ... and scan m's are served now
    reg.close()


def _saved(reg):
    """(status of lii_publish_saved, the cloud, status of lii_publish_saved_intensity, the intensities)"""
    n = C.c_int32(0)
    reg.L.lii_publish_saved(reg.h, None, 0, C.byref(n), 0)
    cloud = np.zeros((max(n.value, 1), 4), np.float32)
    rc = reg.L.lii_publish_saved(reg.h, cloud.ctypes.data_as(C.c_void_p), len(cloud), C.byref(n), 0)
    ni = C.c_int32(0)
    reg.L.lii_publish_saved_intensity(reg.h, None, 0, C.byref(ni))
    it = np.zeros(max(ni.value, 1), np.float32)
    rci = reg.L.lii_publish_saved_intensity(reg.h, it.ctypes.data_as(C.c_void_p), len(it), C.byref(ni))
    return rc, cloud[:n.value], rci, it[:ni.value]


def test_save_buffer_keeps_cloud_and_intensity_aligned():
    scans = [_take(n, True) for n in (1500, 1000, 1200)]
    intens = [_floats(len(s), 70 + k) for k, s in enumerate(scans)]
    reg = _registrar()
    reg.publish_set(DENSE | INTENSITY, to_host=True, save_capacity=1500 + 1000 + 1199)  # the third scan does not fit
    st = _state("poses")
    dense = []
    for m, s in enumerate(scans):
        reg.scan_upload(s)
        if m != 1:
            reg.scan_intensity_upload(intens[m])  # the middle scan is registered without intensities: zeros
        _register(reg, "poses", st, leaf=0.2, max_iterations=3, scan_sorted=True)
        dense.append(reg.publish_fetch(DENSE))
        if m == 1:
            assert _code(lambda: reg.publish_fetch_intensity(DENSE)) == STATE  # (the registered scan had none)
            rc, cloud, rci, it = _saved(reg)
            assert rc == 0 and rci == 0 and len(cloud) == len(it) == 2500
    rc, cloud, rci, it = _saved(reg)
    assert rc == CAPACITY and rci == CAPACITY  # sticky: a scan was not appended
    assert len(cloud) == len(it) == 2500
    assert np.array_equal(_bits(cloud), _bits(np.concatenate(dense[:2])))
    assert np.array_equal(_bits(it), _bits(np.r_[intens[0], np.zeros(1000, np.float32)]))
    assert _code(lambda: reg.publish_saved(clear=True)) == CAPACITY
    rc, cloud, rci, it = _saved(reg)
    assert rc == 0 and rci == 0 and len(cloud) == 0 and len(it) == 0  # `clear` empties both
    # ... and the next scan lands at offset 0 in both
    reg.scan_upload(scans[2])
    reg.scan_intensity_upload(intens[2])
    _register(reg, "poses", st, leaf=0.2, max_iterations=3, scan_sorted=True)
    rc, cloud, rci, it = _saved(reg)
    assert rc == 0 and len(cloud) == 1200 and np.array_equal(_bits(it), _bits(intens[2])) and np.array_equal(_bits(cloud), _bits(reg.publish_fetch(DENSE)))
    reg.close()


def test_refusals():
    import lidar_imu_init_amd as lii
    reg = _registrar()
    scan, inten = _take(1000, True), _floats(1000, 80)
    assert _code(lambda: reg.scan_intensity_upload(inten)) == STATE  # no scan
    assert _code(lambda: reg.scan_intensity_download(0)) == STATE
    reg.scan_upload(scan)
    assert _code(lambda: reg.scan_intensity_upload(inten[:999])) == INVALID  # a count mismatch
    assert _code(lambda: reg.scan_intensity_set_device(reg.device_intensity(np.r_[inten, inten]))) == INVALID
    assert _code(lambda: reg.scan_intensity_download(2)) == INVALID
    assert _code(lambda: reg.publish_set(INTENSITY)) == INVALID  # bit 16 alone
    assert _code(lambda: reg.publish_set(EFFECT | INTENSITY)) == INVALID
    assert _code(lambda: reg.publish_set(32 | DENSE)) == INVALID
    reg.publish_set(DENSE | DOWN | EFFECT, to_host=True)  # an order without the bit
    reg.scan_intensity_upload(inten)
    st = _state("poses")
    _register(reg, "poses", st, leaf=0.2, max_iterations=3, scan_sorted=True)
    assert _code(lambda: reg.publish_fetch_intensity(DENSE)) == STATE
    reg.publish_set(DENSE | INTENSITY, to_host=True)
    assert _code(lambda: reg.publish_fetch_intensity(DENSE)) == STATE  # no registration since the order
    _register(reg, "poses", st, leaf=0.2, max_iterations=3, scan_sorted=True)
    assert np.array_equal(_bits(reg.publish_fetch_intensity(DENSE)), _bits(inten))
    assert _code(lambda: reg.publish_fetch_intensity(EFFECT)) == INVALID
    assert _code(lambda: reg.publish_fetch_intensity(BODY)) == STATE  # a cloud that was not ordered
    assert _code(lambda: reg.publish_fetch_intensity(DOWN)) == STATE
    assert _code(lambda: reg.publish_fetch_intensity(3)) == INVALID and _code(lambda: reg.publish_fetch(INTENSITY)) == INVALID
    assert _code(lambda: reg.publish_saved_intensity()) == STATE  # no save buffer
    # whatever replaces the scan detaches the intensities
    reg.scan_set_device(reg.device_scan(scan))
    assert _code(lambda: reg.scan_intensity_download(0)) == STATE
    reg.scan_intensity_upload(inten)
    reg.scan_upload_next(np.ascontiguousarray(scan))
    reg.scan_advance()
    assert _code(lambda: reg.scan_intensity_download(0)) == STATE
    reg.scan_intensity_upload(inten)
    _register(reg, "poses", st, leaf=0.2, max_iterations=3, scan_sorted=True, scan_dev=reg.device_scan(scan))  # the job adopts scan_dev
    assert _code(lambda: reg.scan_intensity_download(0)) == STATE and _code(lambda: reg.publish_fetch_intensity(DENSE)) == STATE
    reg.close()
    # LII_TEST=host_solve: the attaching calls and the bit are refused, as publish is
    hs = _registrar(LII_TEST="host_solve")
    hs.scan_upload(scan)
    assert _code(lambda: hs.scan_intensity_upload(inten)) == STATE
    assert _code(lambda: hs.scan_intensity_set_device(hs.device_intensity(inten))) == STATE
    assert _code(lambda: hs.ingest_set_intensity(True)) == STATE
    assert _code(lambda: hs.publish_set(DENSE | INTENSITY)) == STATE
    hs.close()
    # a communicator attached (one rank is enough to attach one)
    cm = _registrar()
    cm.comm_init(1, 0, cm.comm_unique_id(), "rccl")
    cm.scan_upload(scan)
    assert _code(lambda: cm.scan_intensity_upload(inten)) == STATE
    assert _code(lambda: cm.scan_intensity_set_device(cm.device_intensity(inten))) == STATE
    assert _code(lambda: cm.ingest_set_intensity(True)) == STATE
    assert _code(lambda: cm.publish_set(DENSE | INTENSITY)) == STATE
    cm.close()


# ------------------------------------------------------------------------------------------------ nothing changes for others
def _launches(reg):
    return {k: v[1] for k, v in reg.kernel_profile()[0].items()}


def test_a_scan_without_intensity_is_registered_as_before():
    """One handle: the per-kind launch counts (lii_set_profiling(h, 3)) of a registration without intensity are the same before and after
    a registration with it; state, report and the four published clouds of the registration without are those of a fresh handle."""
    scan, inten = _take(5000, True), _floats(5000, 90)

    def run(reg, with_int):
        reg.set_profiling(1)
        reg.set_profiling(3)
        st = _state("poses")
        reg.scan_upload(scan)
        if with_int:
            reg.scan_intensity_upload(inten)
        rep = _register(reg, "poses", st, leaf=0.2, max_iterations=4, scan_sorted=True)
        clouds = [reg.publish_fetch(c) for c in (DENSE, DOWN, EFFECT, BODY)]
        return _launches(reg), st.pod.tobytes(), (rep["iterations"], rep["searches"], rep["effect_num"], rep["normal_eq"].tobytes()), clouds

    reg = _registrar()
    reg.publish_set(DENSE | DOWN | EFFECT | BODY | INTENSITY, to_host=True)
    run(reg, False)  # (the first scan of a leaf is probed: not the steady state)
    before = run(reg, False)
    with_i = run(reg, True)
    assert np.array_equal(_bits(reg.publish_fetch_intensity(BODY)), _bits(inten))
    after = run(reg, False)
    reg.close()
    print("launches per kind without intensity:", before[0])
    print("launches per kind with intensity attached, DENSE | DOWN | EFFECT | BODY | INTENSITY ordered:", with_i[0])
    assert before[0] == after[0]
    fresh = _registrar()
    fresh.publish_set(DENSE | DOWN | EFFECT | BODY, to_host=True)
    run(fresh, False)
    ref = run(fresh, False)
    fresh.close()
    for got in (before, after, with_i):  # (the intensities ride along: they change nothing of the registration itself)
        assert got[1] == ref[1] and got[2] == ref[2]
        for a, b in zip(got[3], ref[3]):
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))
    assert ref[0] == before[0]
