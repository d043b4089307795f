"""Feature extraction on the device (lii_ingest_set_features: give_feature / plane_judge / edge_jump_judge behind the whole-message ingest)
against the reference's own output (tests/golden/features/reference_features.npz, from the unmodified src/preprocess.cpp) and, where the
reference is undefined, against tests/feature_np.py.  Every comparison is BIT-IDENTICAL: every operation on the path is a correctly
rounded IEEE basic operation in a fixed order, so there is no tolerance - a mismatch is traced to its operation."""
import os
import sys

import numpy as np
import pytest
import torch  # (before the library is loaded: hipMemGetInfo is read through torch.cuda.mem_get_info, as tests/test_gpu_handle_lifecycle.py reads it)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import feature_cases  # noqa: E402
import feature_np  # noqa: E402
from harness import synth, wire  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(HERE, "golden", "features", "reference_features.npz")


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in feature_cases.fixture_cases()}


@pytest.fixture(scope="module")
def reg():
    import lidar_imu_init_amd as lii
    r = lii.Registrar(max_scan_points=20_000, max_map_points=1000, filter_size_map=0.2)
    r.ingest_set_features(True)
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ingest(reg, c, cut=0, begin=False):
    if c["livox"]:
        args = (c["raw"], c["n"], c["fields"], c["n_scans"], c["pfn"], c["blind"], c["stamp"], cut, 100)
        if begin:
            return reg.ingest_livox_begin(*args)
        return reg.ingest_livox(*args)
    args = (c["raw"], c["n"], c["fields"], c["lidar_type"], c["n_scans"], c["pfn"], c["blind"], c["stamp"], cut, 100)
    if begin:
        return reg.ingest_pcl2_begin(*args)
    return reg.ingest_pcl2(*args)


def _frames(reg, info):
    out = []
    for k in range(len(info)):
        reg.frame_select(k)
        out.append(reg.scan_download(0).copy())
    return out


def _check_against(reg, info, c, surf, corn, n_lines=None):
    """frame table, frame points, corners"""
    name = c["name"]
    if len(surf) == 0:
        assert info == [], name
    else:
        assert len(info) == 1 and info[0][0] == c["stamp"] and info[0][1] == 0 and info[0][2] == len(surf), (name, info, len(surf))
        pts = _frames(reg, info)[0]
        if not _same(pts[:, :4], surf):
            bad = np.nonzero((_bits(pts[:, :4]) != _bits(surf)).any(1))[0] if pts[:, :4].shape == surf.shape else []
            raise AssertionError((name, "pl_surf differs", pts.shape, surf.shape, list(bad[:5]), pts[bad[:2]], surf[bad[:2]]))
        assert reg.frame_tail_ms[0] == float(surf[-1, 3]), name
    xyzt, inten = reg.ingest_corners()
    assert _same(xyzt, corn[:, [0, 1, 2, 4]]), (name, "pl_corn differs", xyzt.shape, corn.shape)
    assert _same(inten, corn[:, 3]), (name, "pl_corn intensities differ")
    f = reg.ingest_features()
    assert f["on"] and f["n_surf"] == len(surf) and f["n_corn"] == len(corn), (name, f)
    if n_lines is not None:
        assert f["n_lines"] == n_lines, (name, f, n_lines)


def test_fixture_cases_bit_identical(reg, fixture, cases):
    """Every fixture case through lii_ingest_livox / lii_ingest_pcl2: frame table, frame points, corners - the reference's bits."""
    assert list(fixture["names"]) == list(cases)
    for name, c in cases.items():
        assert fixture[name + "/raw"].tobytes() == c["raw"], name
        info = _ingest(reg, c)
        _check_against(reg, info, c, fixture[name + "/surf"], fixture[name + "/corn"])


def test_overlapped_forms_two_messages_under_way(reg, fixture, cases):
    pairs = [("avia_6x700_pfn3", "ouster_16x64_pfn3"), ("velo_16x129_pfn3_notime", "avia_6x129_pfn1"), ("ouster_128x65_pfn1", "velo_16x64_pfn4")]
    for a, b in pairs:
        _ingest(reg, cases[a], begin=True)
        _ingest(reg, cases[b], begin=True)
        for name in (a, b):
            info = reg.ingest_end()
            _check_against(reg, info, cases[name], fixture[name + "/surf"], fixture[name + "/corn"])


def test_where_the_reference_is_undefined(reg):
    """Kept points with range < blind, a line blind throughout, an empty OUSTER line: the library's definitions (include/liinit_hip.h),
    restated in tests/feature_np.py."""
    seen_below, seen_blind_line = 0, 0
    for c in feature_cases.extra_cases():
        r = feature_np.features(c)
        lines = [feature_np._Line(xyz, c["lidar_type"], c["blind"]) for xyz, _, _ in feature_np.collect(c)]
        seen_below += sum(int((L.range < c["blind"]).sum()) for L in lines)
        seen_blind_line += sum(1 for L in lines if L.n > 0 and (L.range < c["blind"]).all())
        if c["name"].endswith("_empty_line"):
            assert lines[3].n == 0
        info = _ingest(reg, c)
        _check_against(reg, info, c, r["surf"], r["corn"], r["n_lines"])
    assert seen_below > 0 and seen_blind_line > 0


def test_order_off_is_the_library_as_it_was(cases):
    """Order off: the frames of a handle that was told `off` equal those of a handle that never heard of the order, no corners, and the
    device memory the two hold (hipMemGetInfo) is the same."""
    import lidar_imu_init_amd as lii
    used, frames = [], []
    for told in (False, True, False, True):
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        r = lii.Registrar(max_scan_points=20_000, max_map_points=1000, filter_size_map=0.2)
        try:
            if told:
                r.ingest_set_features(True)
                r.ingest_set_features(False)
            got = []
            for name in ("ouster_128x65_pfn1", "avia_6x700_pfn3", "velo_16x129_pfn3_notime"):
                info = _ingest(r, cases[name])
                got.append((info, r.frame_tail_ms, _frames(r, info)))
                xyzt, inten = r.ingest_corners()
                assert len(xyzt) == 0 and len(inten) == 0
                f = r.ingest_features()
                assert f == dict(on=False, n_surf=0, n_corn=0, n_lines=0)
            torch.cuda.synchronize()
            free1, _ = torch.cuda.mem_get_info()
            used.append(free0 - free1)
            frames.append(got)
        finally:
            r.close()
    print("device memory a handle holds after three plain ingests (never told, told off, never told, told off):", used)
    assert used[2] == used[3], used  # (the first pair warms the runtime's own pools)
    for (ia, ta, fa), (ib, tb, fb) in zip(frames[2], frames[3]):
        assert ia == ib and ta == tb and len(fa) == len(fb) and all(_same(x, y) for x, y in zip(fa, fb))
    # the plain frame is the decimated cloud, not pl_surf
    assert frames[2][0][0][0][2] != 7618
    # ... and the reading sees the buffers when they do come: with the first message ingested under the order
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    r = lii.Registrar(max_scan_points=20_000, max_map_points=1000, filter_size_map=0.2)
    try:
        r.ingest_set_features(True)
        for name in ("ouster_128x65_pfn1", "avia_6x700_pfn3", "velo_16x129_pfn3_notime"):
            assert len(_ingest(r, cases[name])) == 1
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info()
    finally:
        r.close()
    print("... and after the same three under the order:", free0 - free1)
    assert free0 - free1 > used[2]


def test_order_on_leaves_cut_messages_and_l515_alone(reg, cases):
    import lidar_imu_init_amd as lii
    plain = lii.Registrar(max_scan_points=20_000, max_map_points=1000, filter_size_map=0.2)
    try:
        for name in ("velo_16x129_pfn3_notime", "ouster_16x129_pfn4", "avia_6x700_pfn3"):
            a, b = _ingest(reg, cases[name], cut=3), _ingest(plain, cases[name], cut=3)
            assert a == b and len(a) >= 1, name
            assert reg.frame_tail_ms == plain.frame_tail_ms
            assert all(_same(x, y) for x, y in zip(_frames(reg, a), _frames(plain, b))), name
            assert len(reg.ingest_corners()[0]) == 0 and reg.ingest_features()["n_surf"] == 0
        xyz = np.frombuffer(cases["ouster_16x129_pfn4"]["raw"], wire.DTYPES[wire.OUSTER])
        xyz = np.stack([xyz["x"], xyz["y"], xyz["z"]], -1)
        raw = wire.pack_pcl2(wire.L515, xyz, None, None, 5.0)
        args = (raw, len(xyz), wire.pc2_fields(wire.L515), wire.L515, 16, 2, 1.0, 5.0, 0, 100)
        a, b = reg.ingest_pcl2(*args), plain.ingest_pcl2(*args)
        assert a == b and len(a) == 1
        assert _same(_frames(reg, a)[0], _frames(plain, b)[0])
        assert len(reg.ingest_corners()[0]) == 0
    finally:
        plain.close()


def test_feature_frame_intensities_are_zero(fixture, cases):
    import lidar_imu_init_amd as lii
    r = lii.Registrar(max_scan_points=20_000, max_map_points=1000, filter_size_map=0.2)
    try:
        r.ingest_set_features(True)
        r.ingest_set_intensity(True)
        for name in ("velo_16x65_pfn1", "avia_6x129_pfn1"):
            info = _ingest(r, cases[name])
            _check_against(r, info, cases[name], fixture[name + "/surf"], fixture[name + "/corn"])
            r.frame_select(0)
            inten = r.scan_intensity_download(0)
            assert len(inten) == info[0][2] and not _bits(inten).any(), name  # all +0.0f: the reference's `ap`
    finally:
        r.close()


def _room_map(step=0.15):
    """The scene of tests/feature_cases.py as a map: three walls, floor, ceiling, the box face."""
    u = np.arange(-10.0, 10.0 + 1e-9, step)
    z = np.arange(-3.0, 3.5 + 1e-9, step)
    def grid(a, b):
        A, B = np.meshgrid(a, b, indexing="ij")
        return A.reshape(-1), B.reshape(-1)
    out = []
    a, b = grid(u, z)
    out += [np.stack([np.full_like(a, 10.0), a, b], -1), np.stack([np.full_like(a, -10.0), a, b], -1), np.stack([a, np.full_like(a, -10.0), b], -1)]
    a, b = grid(u, u)
    out += [np.stack([a, b, np.full_like(a, -3.0)], -1), np.stack([a, b, np.full_like(a, 3.5)], -1)]
    a, b = grid(np.arange(-2.0, 2.0 + 1e-9, step), z)
    out.append(np.stack([np.full_like(a, 6.0), a, b], -1))
    return np.ascontiguousarray(np.concatenate(out), np.float32)


def test_feature_frame_registers_like_the_uploaded_pl_surf(fixture, cases, oracle):
    """One registration end to end: the feature frame handed to lii_scan_register with scan_sorted = 2, against the state obtained by
    uploading the fixture's pl_surf and registering with the same job."""
    import lidar_imu_init_amd as lii
    from conftest import make_state
    name = "ouster_128x65_pfn1"
    map_pts = _room_map()
    st0 = oracle.state_boxplus(make_state(oracle), np.r_[0.002, -0.002, 0.003, 0.02, -0.02, 0.01, np.zeros(18)])
    states, reps = [], []
    for through_ingest in (True, False):
        r = lii.Registrar(max_scan_points=20_000, max_map_points=len(map_pts) + 1000, filter_size_map=0.15)
        try:
            r.map_build(map_pts)
            if through_ingest:
                r.ingest_set_features(True)
                info = _ingest(r, cases[name])
                assert len(info) == 1
                r.frame_select(0)
            else:
                r.scan_upload(np.ascontiguousarray(fixture[name + "/surf"], np.float32))
            s = lii.State(st0)
            rep = r.scan_register(s, lii.State(st0), leaf=0.1, max_iterations=5, imu_en=False, scan_sorted=2)
            states.append(np.array(s.pod, np.float64).copy())
            reps.append((rep["iterations"], rep["effect_num"]))
        finally:
            r.close()
    assert reps[0] == reps[1] and reps[0][1] > 500, reps
    assert states[0].tobytes() == states[1].tobytes()
    assert np.linalg.norm(states[0] - np.asarray(st0, np.float64).reshape(-1)[:len(states[0])]) > 0  # (the update moved the state)
