"""lii_scan_register_cv - Process() with imu_en == false (src/IMU_Processing.hpp:212-266) + the per-scan sequence in one call, the
constant-velocity propagation riding in the de-skew launch (lii_scan.hip: k_deskew_cv_prop) - against

  1. the UNMODIFIED reference header, as recorded in tests/golden/imu/reference_cv_process.npz (always) and as oracle/_ref/libref_imu.so
     computes it live (where it is built): cases A (4 097 points: the last scan workgroup holds one point), B (4 096 points, zero rates,
     first frame: Exp's small-angle branch) and C (A permuted, scan_sorted = 0: the time-extent form);
  2. this library's two-call path - lii_cv_propagate, then lii_scan_register(undistort = 2) - on the same handle, scan and map: the same
     device code on the same inputs, so every output is bit-equal;
  3. the oracle chain (header -> oracle.voxel_grid -> Tree.iekf_update);
  4. the header again over three consecutive scans with the map updated inside the call;
  5. the rules of include/liinit_hip.h.

Bounds.  Propagated state[:36] within 1e-12 absolute, covariance within 1e-12 max|cov| (tests/test_gpu_imu_propagate.py:98-99: the
header forms dt as a difference of absolute stamps).  De-skewed cloud: stamps equal, coordinates within 3 float ulp - the de-skew's
2 ulp against the header (tests/test_gpu_scan_ops.py) plus one for the rounding of the end rotation, the argument of
test_scan_register_imu_equals_the_host_fed_path.  Final state against the oracle chain: the bounds of tests/test_gpu_imu_propagate.py:223-225."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
LEAF, MAX_IT = 0.1, 5
_cache = {}


def _fx():
    import make_cv_process_fixture as M
    return M


def _case(name):
    if name not in _cache:
        _cache[name] = _fx().load(name)
    return _cache[name]


def _map_pts():
    if "map" not in _cache:
        _cache["map"] = _fx().hall().surface_points(0.15, noise=0.01, seed=7)
    return _cache["map"]


def _registrar(**kw):
    import lidar_imu_init_amd as lii
    return lii.Registrar(**{**dict(max_scan_points=20_000, max_map_points=600_000, filter_size_map=0.15), **kw})


def _ulp_diff(a, b):  # tests/test_gpu_scan_ops.py
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def _check_against_header(tag, prop_pod, cloud, ref_state, ref_cloud):
    d_state = float(np.abs(prop_pod[:36] - ref_state[:36]).max())
    d_cov = float(np.abs(prop_pod[36:] - ref_state[36:]).max() / np.abs(ref_state[36:]).max())
    order = np.argsort(cloud[:, 3], kind="stable")  # (the header hands its cloud over sorted by stamp; the stamps are distinct)
    got = cloud[order]
    stamps_equal = np.array_equal(got[:, 3], ref_cloud[:, 3])
    ulp = int(_ulp_diff(got[:, :3], ref_cloud[:, :3]).max()) if stamps_equal else -1
    print(f"{tag}: max|dstate[:36]| {d_state:.2e}  max|dcov|/max|cov| {d_cov:.2e}  cloud max {ulp} ulp over {len(cloud)} points")
    assert d_state <= 1e-12
    assert d_cov <= 1e-12
    assert stamps_equal
    assert ulp <= 3
    return d_state, d_cov, ulp


def _register(reg, c, state, *, sorted_, leaf=LEAF, scan_dev=None, map_update=False):
    return reg.register_cv(c["dt"], c["cov_gyr_scale"], c["cov_acc_scale"], state, leaf=leaf, max_iterations=MAX_IT, scan_sorted=sorted_,
                           scan_dev=scan_dev, map_update=map_update)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_scan_register_cv_equals_the_reference_header(name):
    import lidar_imu_init_amd as lii
    from oracle import oracle as O
    c = _case(name)
    refs = [("fixture", c["out_state"], c["out_points"])]
    if O.ref_imu_lib() is not None:
        st, cloud = _fx().run_header(c)
        refs.append(("live header", st, cloud))
    reg = _registrar()
    reg.map_build(_map_pts())
    reg.scan_upload(c["pts"])
    st0 = lii.State(c["state"])
    st, prop, rep = _register(reg, c, st0.copy(), sorted_=(name != "C"))
    cloud = reg.scan_download(0)
    print(f"case {name}: report", {k: rep[k] for k in ("iterations", "searches", "effect_num")})
    for tag, rs, rc in refs:
        _check_against_header(f"lii_scan_register_cv {name} vs {tag}", prop.pod, cloud, rs, rc)
    if name != "C":
        assert np.array_equal(cloud[:, 3], c["pts"][:, 3])  # (input order kept)
    assert rep["effect_num"] > 100
    reg.close()


@pytest.mark.parametrize("leaf", [0.1, 0.0])
@pytest.mark.parametrize("from_dev", [False, True])
def test_scan_register_cv_is_bit_equal_to_the_two_call_path(leaf, from_dev):
    """lii_cv_propagate + lii_scan_register(undistort = 2) on the same handle, scan and map.  Both sides run the same device code on the
    same inputs: any difference is a bug, the bound is zero."""
    import lidar_imu_init_amd as lii
    for name, sorted_ in (("A", True), ("B", True), ("C", False)):
        c = _case(name)
        reg = _registrar()
        reg.map_build(_map_pts())
        st0 = lii.State(c["state"])
        dev = reg.device_scan(c["pts"]) if from_dev else None
        # ---- one call
        if not from_dev:
            reg.scan_upload(c["pts"])
        st_a, prop_a, rep_a = _register(reg, c, st0.copy(), sorted_=sorted_, leaf=leaf, scan_dev=dev)
        cloud_a = reg.scan_download(0)
        # ---- two calls
        if not from_dev:
            reg.scan_upload(c["pts"])
        prop_b = reg.propagate_cv(c["dt"], c["cov_gyr_scale"], c["cov_acc_scale"], st0)
        st_b = prop_b.copy()
        rep_b = reg.scan_register(st_b, prop_b, cv=True, leaf=leaf, max_iterations=MAX_IT, scan_sorted=sorted_, scan_dev=dev)
        cloud_b = reg.scan_download(0)
        ra, rb = [tuple(r[k] for k in ("iterations", "searches", "effect_num")) for r in (rep_a, rep_b)]
        print(f"case {name} leaf {leaf} scan_dev {from_dev}: reports {ra} / {rb}; propagated state differs in "
              f"{int((prop_a.pod != prop_b.pod).sum())} doubles, cloud in {int((cloud_a != cloud_b).sum())} floats, final state in "
              f"{int((st_a.pod != st_b.pod).sum())} doubles")
        assert np.array_equal(prop_a.pod, prop_b.pod)
        assert np.array_equal(cloud_a, cloud_b)
        assert ra == rb
        assert np.array_equal(st_a.pod, st_b.pod)
        reg.close()


def test_scan_register_cv_against_the_oracle_chain(oracle):
    import lidar_imu_init_amd as lii
    c = _case("A")
    reg = _registrar()
    reg.map_build(_map_pts())
    reg.scan_upload(c["pts"])
    st_a, _, rep_a = _register(reg, c, lii.State(c["state"]), sorted_=True)
    reg.close()
    tree = oracle.Tree("oracle")
    tree.build(_map_pts())
    body, _ = oracle.voxel_grid(c["out_points"], LEAF)
    want = tree.iekf_update(body, c["out_state"], c["out_state"], max_iterations=MAX_IT, imu_en=False)
    tree.close()
    w = lii.State(want["state"])
    dp = float(np.linalg.norm(w.pos_end - st_a.pos_end))
    dth = float(np.linalg.norm(oracle.log_so3(w.rot_end.T @ st_a.rot_end)))
    d_pe = float(np.abs(w.pod[:24] - st_a.pod[:24]).max())
    d_rest = float(np.abs(w.pod[24:36] - st_a.pod[24:36]).max())
    d_cov = float(np.abs(st_a.cov - w.cov).max() / np.abs(w.cov).max())
    print(f"final state vs the oracle chain: |dp| {dp:.2e} m |dtheta| {dth:.2e} rad pose+extrinsic {d_pe:.2e} other states {d_rest:.2e} "
          f"max|dcov|/max|cov| {d_cov:.2e}; iterations {rep_a['iterations']} / {want['iters']}")
    assert rep_a["iterations"] == want["iters"]
    assert dp <= 1e-6 and dth <= 1e-7 and d_pe <= 1e-7 and d_rest <= 1e-5
    assert d_cov <= 5e-4


def test_three_lo_scans_stay_with_the_header():
    """Three consecutive LO scans (sub-frames 0 - 2 of the fixture's stream, 4 097 points each) with map_update = 1.  At every scan the
    header is run from the GPU's previous state, so nothing compounds.  Between two scans the host does what the LO loop does with the
    updated pose (src/laserMapping.cpp:1137-1143): vel_end and bias_g become the rates of the motion - here the trajectory's own."""
    import lidar_imu_init_amd as lii
    from oracle import oracle as O
    if O.ref_imu_lib() is None:
        pytest.skip("oracle/_ref/libref_imu.so not built (needs the reference tree at build time)")
    M = _fx()
    c = _case("A")
    reg = _registrar()
    reg.map_build(_map_pts())
    st = lii.State(c["state"])
    worst = np.zeros(3)
    for k in range(3):
        pts = c["pts"] if k == 0 else M.make_scan(k)
        assert len(pts) == M.N_A
        ck = dict(c, pts=pts, state=st.pod.copy())
        ref_state, ref_cloud = M.run_header(ck)
        dev = reg.device_scan(pts)
        st, prop, rep = _register(reg, ck, st, sorted_=True, scan_dev=dev, map_update=True)
        cloud = reg.scan_download(0)
        worst = np.maximum(worst, _check_against_header(f"scan {k}", prop.pod, cloud, ref_state, ref_cloud))
        print(f"scan {k}: report", {q: rep[q] for q in ("iterations", "searches", "effect_num")})
        assert rep["effect_num"] > 100, rep
        rates = M.lo_state(M.T_BEG + (k + 1) * M.SWEEP, True)
        st.vel_end[:] = rates.vel_end
        st.bias_g[:] = rates.bias_g
    print("three scans, worst: state %.2e cov (rel) %.2e cloud %d ulp" % tuple(worst))
    reg.close()


def test_rules_of_lii_scan_register_cv():
    import ctypes as C
    import lidar_imu_init_amd as lii
    c = _case("A")
    INVALID, STATE = -1, -5
    st0 = lii.State(c["state"])
    kw = dict(leaf=LEAF, max_iterations=MAX_IT, scan_sorted=True)

    def refused(reg, want, **over):
        st = st0.copy()
        args = dict(dt=c["dt"], g=c["cov_gyr_scale"], a=c["cov_acc_scale"])
        args.update({k: over.pop(k) for k in ("dt", "g", "a") if k in over})
        with pytest.raises(lii.LIIError) as e:
            reg.register_cv(args["dt"], args["g"], args["a"], st, **{**kw, **over})
        assert e.value.code == want, (e.value.code, want, over)
        assert np.array_equal(st.pod, st0.pod)  # a refused call leaves `state` as it was

    reg = _registrar()
    reg.map_build(_map_pts())
    refused(reg, STATE)  # no scan
    reg.scan_upload(c["pts"])
    refused(reg, INVALID, undistort=1)
    refused(reg, INVALID, undistort=0)
    refused(reg, INVALID, imu_poses=np.zeros((3, 22)))
    refused(reg, INVALID, g=None)
    refused(reg, INVALID, a=None)
    refused(reg, INVALID, dt=float("nan"))
    refused(reg, INVALID, dt=float("inf"))
    # n_imu_poses != 0 with imu_poses == NULL
    from lidar_imu_init_amd import api
    job = api.lii_scan_job()
    job.struct_size, job.undistort, job.leaf, job.n_imu_poses, job.scan_sorted = C.sizeof(api.lii_scan_job), 2, LEAF, 3, 1
    job.opts = api.lii_iekf_opts(MAX_IT, 0)
    st, rep = st0.copy(), api.lii_iekf_report()
    g, a = np.ascontiguousarray(c["cov_gyr_scale"]), np.ascontiguousarray(c["cov_acc_scale"])
    assert reg.L.lii_scan_register_cv(reg.h, C.byref(job), c["dt"], g.ctypes.data, a.ctypes.data, st.pod.ctypes.data, None, C.byref(rep)) == INVALID
    assert np.array_equal(st.pod, st0.pod)
    # a communicator attached
    reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")
    refused(reg, STATE)
    reg.comm_destroy()
    # profiling mode 3: one successful call is one de-skew launch and no propagate launch
    reg.set_profiling(1)
    reg.set_profiling(3)
    st_ok, prop_ok, rep_ok = reg.register_cv(c["dt"], c["cov_gyr_scale"], c["cov_acc_scale"], st0.copy(), **kw)
    reg.synchronize()
    kp, n_scans = reg.kernel_profile()
    print("profile of one call:", {k: v for k, v in kp.items()})
    assert n_scans == 1 and kp["deskew"][1] == 1 and kp["propagate"][1] == 0
    reg.set_profiling(0)
    # a job that asks for no propagated state registers alike
    reg.scan_upload(c["pts"])
    st_np, none, _ = reg.register_cv(c["dt"], c["cov_gyr_scale"], c["cov_acc_scale"], st0.copy(), want_propagated=False, **kw)
    assert none is None and np.array_equal(st_np.pod, st_ok.pod)
    reg.close()
    # no map: what lii_scan_register returns (a status, or LII_OK with a report)
    def outcome(fn):
        try:
            return (0, fn()["effect_num"])
        except lii.LIIError as e:
            return (e.code, None)

    reg = _registrar()
    prop = reg.propagate_cv(c["dt"], c["cov_gyr_scale"], c["cov_acc_scale"], st0)
    reg.scan_upload(c["pts"])
    plain = outcome(lambda: reg.scan_register(prop.copy(), prop, cv=True, **kw))
    reg.scan_upload(c["pts"])
    st_nm = st0.copy()
    fused = outcome(lambda: reg.register_cv(c["dt"], c["cov_gyr_scale"], c["cov_acc_scale"], st_nm, **kw)[2])
    print("no map: lii_scan_register", plain, " lii_scan_register_cv", fused)
    assert fused == plain
    if fused[0] != 0:
        assert np.array_equal(st_nm.pod, st0.pod)
    reg.close()
    # LII_TEST=host_solve: refused; LII_TEST=no_fast: lii_cv_propagate + the general path, the same results
    for env in ("host_solve", "no_fast"):
        old = os.environ.get("LII_TEST")
        os.environ["LII_TEST"] = env
        try:
            reg = _registrar()
        finally:
            os.environ.pop("LII_TEST", None)
            if old is not None:
                os.environ["LII_TEST"] = old
        reg.map_build(_map_pts())
        reg.scan_upload(c["pts"])
        if env == "host_solve":
            refused(reg, STATE)
        else:
            st_nf, prop_nf, rep_nf = reg.register_cv(c["dt"], c["cov_gyr_scale"], c["cov_acc_scale"], st0.copy(), **kw)
            assert np.array_equal(prop_nf.pod, prop_ok.pod) and np.array_equal(st_nf.pod, st_ok.pod)
            assert (rep_nf["iterations"], rep_nf["effect_num"]) == (rep_ok["iterations"], rep_ok["effect_num"])
        reg.close()
