"""lii_point_noise_set on the device: every selected point weighted by its own R_inv_i = 1 / sigma^2_i (range along the ray, bearing
across it: calcBodyVar, src/laserMapping.cpp:158-181, :1039-1042), against the per-point numpy reference (tests/point_noise_np.py on top of
tests/plane_rows_np.py).

The method is tests/test_gpu_plane_rows.py's: lii_iekf_iterate returns the 91 sums of a scan; with one live point among filler points whose
rows are exactly zero the sums ARE that point's row - out[0:78] = R_inv_i h h^T, out[78:90] = R_inv_i h z - and no summation order is
involved.  The map is plane_rows_np's set of isolated clusters plus family K (queries with z = 0 in the IMU frame, where the reference's
own formula is not finite).

Tolerances.  One point's row: plane_rows_np's own (DEVICE_FACTOR x DISC, relative to R_inv_i |h|^2 and R_inv_i |h| |z|) plus 8 x 2^-52 for
the weight's own double operations (two reciprocals, the square root, its square, two products); the same exclusion rule and cap.  Sums of
many points: that per-row tolerance times sum R_inv_i |h_i|^2 (sum R_inv_i |h_i| |z_i| for the z column).  sqrt(R_inv_i) as a float: 1 ulp.
The resident loop against LII_TEST=host_solve: 1e-6 m / 1e-7 (rotation, element-wise), the bound the device algebra is held to against
the host-driven loop everywhere (tests/test_gpu_launch_plan.py).  Run with -s for the worst observed fractions (profiles/point_noise.md).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import plane_rows_np as pr
import point_noise_np as pn

pytestmark = pytest.mark.gpu

TOL_HH = pr.DEVICE_FACTOR * pr.DISC["hh"] + pn.W_EPS
TOL_HZ = pr.DEVICE_FACTOR * pr.DISC["hz"] + pn.W_EPS
INVALID, STATE, CAPACITY = -1, -5, -4
SUM_CFG = ("lio", True)
EFFECT_CONSTANT = np.float32(np.sqrt(np.float64(1000.0)))  # src/laserMapping.cpp:1050-1051


def _code(fn, *a, **kw):
    import lidar_imu_init_amd as lii
    try:
        fn(*a, **kw)
        return 0
    except lii.LIIError as e:
        return e.code


def _registrar(env=None, **kw):
    import lidar_imu_init_amd as lii
    old = os.environ.get("LII_TEST")
    os.environ.pop("LII_TEST", None)
    if env:
        os.environ["LII_TEST"] = env
    try:
        return lii.Registrar(**kw)
    finally:
        os.environ.pop("LII_TEST", None)
        if old is not None:
            os.environ["LII_TEST"] = old


@pytest.fixture(scope="module")
def cs():
    return pn.noise_cases()


@pytest.fixture(scope="module")
def refs(cs, oracle):
    """Per CONFIGS entry, computed once: the queries' body points, the two states, the numpy rows of the search pass and of the pass on
    cached planes at state [+] MOVE, and the points' weights in both."""
    st0 = oracle.state_init()
    out = {}
    for pname, imu_en in pr.CONFIGS:
        pose = pr.POSES[pname]
        ids, body = cs.bodies(pname)
        pose2, pod2 = pn.moved_pose(pname, oracle.state_boxplus, st0)
        ref = cs.reference(pname, imu_en)
        ref2 = cs.reference(pname, imu_en, pose=pose2, cached=ref)
        fam = np.array([cs.nh[cs.queries[k]["nh"]]["family"] for k in ids])
        out[(pname, imu_en)] = dict(ids=ids, body=body, pod=pose.pod(st0), pod2=pod2, pose=pose, pose2=pose2, ref=ref, ref2=ref2, fam=fam,
                                    w=np.array([pn.weight_of(pose, r) for r in ref]), w2=np.array([pn.weight_of(pose2, r) for r in ref2]))
    return out


def _cluster_registrar(cs, max_scan_points):
    reg = _registrar(max_scan_points=max_scan_points, max_map_points=4096, filter_size_map=0.15)
    reg.map_build(cs.map)
    assert reg.map_size() == len(cs.map)
    return reg


@pytest.fixture(scope="module")
def reg(cs):
    r = _cluster_registrar(cs, 2048)
    r.set_point_noise()
    yield r
    r.close()


def run_scan(reg, bodies, pod, pod2, imu_en, noise=True):
    """One search pass at `pod`, then one pass on cached planes at `pod2`: the 91 sums and - under model 1 - the noise buffer of each."""
    import lidar_imu_init_amd as lii
    scan = pr.scan_of(bodies)
    reg.scan_upload(scan)
    n = reg.downsample_skip()
    assert n == len(scan)
    r = dict(out=reg.iekf_iterate(lii.State(pod), True, imu_en))
    if noise:
        r["sq"] = reg.point_noise_download()
        assert r["sq"].shape == (n,) and r["sq"].dtype == np.float32
    r["out2"] = reg.iekf_iterate(lii.State(pod2), False, imu_en)
    if noise:
        r["sq2"] = reg.point_noise_download()
    return r


def _check_row(tag, r, w, f, out, sq, at, worst):
    """The live point's row (and its entry of the noise buffer, every other entry 0) against the numpy reference under its own weight."""
    others = np.arange(len(sq)) != at
    assert not sq[others].any(), (tag, "a filler row has a weight")
    if pr.excluded(r, f):
        worst["left out"] += 1
        return
    assert (sq[at] != 0) == r["selected"], (tag, sq[at], r["selected"], r["margin"])
    assert out[90] == float(r["selected"]), (tag, out[90])
    if not r["selected"]:
        assert not np.any(out), (tag, out)
        return
    want = np.float32(math.sqrt(w))
    assert pn.ulp32_apart(sq[at], want) <= 1, (tag, sq[at], want)
    a, b = pn.group_ratios(out, r, w, TOL_HH, TOL_HZ, f)
    worst["hh"], worst["hz"] = max(worst["hh"], a), max(worst["hz"], b)
    assert a <= 1.0 and b <= 1.0, (tag, a, b, "x the tolerance (out[0:78], out[78:90])", r["margin"])


# ------------------------------------------------------------------------------------------------ 1: one point's row
@pytest.mark.parametrize("key", pr.CONFIGS, ids=lambda k: f"{k[0]}-imu{int(k[1])}")
def test_one_points_row(cs, refs, reg, key):
    c = refs[key]
    pose = c["pose"]
    filler = cs.filler_bodies(key[0], 4)
    worst, worst2 = dict(hh=0.0, hz=0.0, **{"left out": 0}), dict(hh=0.0, hz=0.0, **{"left out": 0})
    ring, near, far = 0, 0, 0
    for k, (r, r2, f) in enumerate(zip(c["ref"], c["ref2"], c["fam"])):
        at = k % 4
        bodies = filler.copy()
        bodies[at] = c["body"][k]
        d = run_scan(reg, bodies, c["pod"], c["pod2"], key[1])
        tag = (key, int(c["ids"][k]), f, cs.queries[c["ids"][k]]["kind"], cs.queries[c["ids"][k]]["tag"])
        _check_row(tag, r, c["w"][k], f, d["out"], d["sq"], at, worst)
        if pr.excluded(r, f) or pr.excluded(r2, f):
            worst2["left out"] += 1
        else:
            _check_row(tag + ("cached",), r2, c["w2"][k], f, d["out2"], d["sq2"], at, worst2)
        if r["selected"]:
            p_i = pn.p_imu_of(pose, r["body"])
            rng = float(np.linalg.norm(p_i))
            ring += p_i[2] == 0.0
            near += rng < 1.0
            far += 55.0 < rng < 70.0
            assert 0.0 < c["w"][k] <= pr.RINV
    for label, ws in (("search pass", worst), ("cached planes", worst2)):
        print(f"\n[one point's row, {label}, {key}] worst device difference / tolerance: out[0:78] {ws['hh']:.3f}, out[78:90] {ws['hz']:.3f}; "
              f"left out {ws['left out']} of {len(c['ref'])}")
        assert ws["left out"] <= pr.EXCLUDE_CAP * len(c["ref"])
    # the sites the model is about: on the ring z_I = 0 exactly, under 1 m, about 60 m.  (Under "lio" the extrinsic moves family J's
    # 0.5 m body points to 0.1 ... 1.1 m in the IMU frame and takes z_I = 0 to within rounding of it: no count is asked of that pose.)
    assert far >= 20 and (key[0] == "lio" or (ring >= 2 and near >= 3)), (ring, near, far)


# ------------------------------------------------------------------------------------------------ 2: zero increments
def test_zero_increments_give_the_constant(cs, refs):
    """range_inc = degree_inc = 0 under model 1: sigma^2 = 1 / laser_point_cov_inv, and every entry is within 8 x 2^-52 (relative to
    rinv |h|^2, rinv |h| |z|) of the entry model 0 gives."""
    key = SUM_CFG
    c = refs[key]
    reg = _cluster_registrar(cs, 64)
    try:
        filler = cs.filler_bodies(key[0], 4)
        picks = [k for k in range(len(c["ref"])) if c["ref"][k]["selected"]][::4]
        worst = 0.0
        for k in picks:
            bodies = filler.copy()
            bodies[k % 4] = c["body"][k]
            reg.clear_point_noise()
            d0 = run_scan(reg, bodies, c["pod"], c["pod2"], key[1], noise=False)
            reg.set_point_noise(0.0, 0.0)
            assert reg.point_noise() == dict(model=1, range_inc=0.0, degree_inc=0.0)
            d1 = run_scan(reg, bodies, c["pod"], c["pod2"], key[1])
            assert d0["out"][90] == d1["out"][90] and d0["out2"][90] == d1["out2"][90]
            for o0, o1, r, sq in ((d0["out"], d1["out"], c["ref"][k], d1["sq"]), (d0["out2"], d1["out2"], c["ref2"][k], d1["sq2"])):
                if not o0[90]:
                    assert not o1.any()
                    continue
                assert pn.ulp32_apart(sq[k % 4], np.float32(math.sqrt(pr.RINV))) <= 1
                hn, z = math.sqrt(float(r["h"] @ r["h"])), abs(r["z"])
                diff = np.abs(o1 - o0)
                frac = max(diff[:78].max() / (pr.RINV * hn * hn), diff[78:90].max() / (pr.RINV * hn * z) if z else 0.0) / pn.W_EPS
                worst = max(worst, frac)
                assert frac <= 1.0, (int(c["ids"][k]), frac)
        print(f"\n[zero increments] {len(picks)} points, worst difference from model 0 / (8 x 2^-52): {worst:.3f}")
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------ 4: sums over workgroups
def _sum_picks(c, n, seed):
    """n live points: selected and rejected queries of the configuration, none excluded, none with a flagged pd2 (its allowance is per point)."""
    ok = [k for k in range(len(c["ref"])) if not pr.excluded(c["ref"][k], c["fam"][k]) and not pr.excluded(c["ref2"][k], c["fam"][k])
          and not pr.pd2_flagged(c["ref"][k], c["fam"][k]) and not pr.pd2_flagged(c["ref2"][k], c["fam"][k])]
    ok = np.array(ok)
    return ok[np.random.default_rng(seed).permutation(len(ok))[np.arange(n) % len(ok)]]


def _check_sums(label, c, picks, d):
    worst = 0.0
    for name, out, ref, w in (("search pass", d["out"], c["ref"], c["w"]), ("cached planes", d["out2"], c["ref2"], c["w2"])):
        rows = np.array([pn.weighted_out(ref[k], w[k]) for k in picks])
        total = np.array([math.fsum(rows[:, t]) for t in range(91)])
        hh = math.fsum(w[k] * float(ref[k]["h"] @ ref[k]["h"]) for k in picks)
        hz = math.fsum(w[k] * math.sqrt(float(ref[k]["h"] @ ref[k]["h"])) * abs(ref[k]["z"]) for k in picks)
        assert out[90] == total[90] == sum(bool(ref[k]["selected"]) for k in picks), (label, name, out[90], total[90])
        diff = np.abs(out - total)
        a = diff[:78].max() / (TOL_HH * hh) if hh else float(diff[:78].max() > 0)
        b = diff[78:90].max() / (TOL_HZ * hz) if hz else float(diff[78:90].max() > 0)
        worst = max(worst, a, b)
        assert a <= 1.0 and b <= 1.0, (label, name, a, b)
    return worst


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_sums_over_workgroups(refs, reg, n):
    c = refs[SUM_CFG]
    picks = _sum_picks(c, n, 7000 + n)
    d = run_scan(reg, c["body"][picks], c["pod"], c["pod2"], SUM_CFG[1])
    sel = np.array([c["ref"][k]["selected"] for k in picks])
    assert np.array_equal(d["sq"] != 0, sel)
    worst = _check_sums(f"n={n}", c, picks, d)
    print(f"\n[sums, n = {n}] selected {int(sel.sum())}, worst difference / tolerance {worst:.3f}")


def test_sums_in_a_cloud_of_more_than_512_workgroups(cs, refs):
    """131 200 points - 513 workgroups, the POSE_V = false instantiations - of which 300 are live; the others lie beside the filler cluster,
    whose plane is rejected: their rows are zero."""
    n, n_live = 131_200, 300
    c = refs[SUM_CFG]
    reg = _cluster_registrar(cs, n)
    try:
        reg.set_point_noise()
        picks = _sum_picks(c, n_live, 7999)
        places = np.sort(np.random.default_rng(8000).choice(n, n_live, replace=False))
        places[0], places[-1] = 0, n - 1
        bodies = cs.filler_bodies(SUM_CFG[0], n)
        bodies[places] = c["body"][picks]
        d = run_scan(reg, bodies, c["pod"], c["pod2"], SUM_CFG[1])
        sel = np.zeros(n, bool)
        sel[places] = [c["ref"][k]["selected"] for k in picks]
        assert np.array_equal(d["sq"] != 0, sel)
        want = np.zeros(n, np.float32)
        want[places] = [np.float32(math.sqrt(c["w"][k])) if c["ref"][k]["selected"] else 0.0 for k in picks]
        assert np.abs(d["sq"].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max() <= 1
        worst = _check_sums(f"n={n}", c, picks, d)
        print(f"\n[sums, n = {n}] selected {int(sel.sum())}, worst difference / tolerance {worst:.3f}")
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------ 3, 5, 6: the resident loop, the effect cloud
@pytest.fixture(scope="module")
def hall_world():
    """A 30 x 24 x 8 m hall seen from near one corner - ranges from under 2 m to over 30 m, every incidence angle -, a 2 048-point scan
    and a start state a few centimetres off."""
    import lidar_imu_init_amd as lii
    from harness import synth
    hall = synth.Hall(size=(30.0, 24.0, 8.0), n_boxes=6, seed=3)
    map_pts = hall.surface_points(0.2, noise=0.01, seed=3)
    R = synth.rot_zyx(0.02, -0.01, 0.3)
    p = np.array([-9.0, -7.0, 0.3])
    scan = synth.make_scan(hall, "tiny", R, p, noise=0.02, seed=5)
    st = lii.State()
    st.rot_end[:] = R @ synth.rot_zyx(0.004, -0.003, 0.005)
    st.pos_end[:] = p + np.array([0.03, -0.02, 0.02])
    st.gravity[:] = [0, 0, -9.81]
    return dict(map=map_pts, scan=scan, st=st)


def _hall_registrar(w, env=None):
    reg = _registrar(env, max_scan_points=4096, max_map_points=max(len(w["map"]), 1000), filter_size_map=0.15)
    reg.map_build(w["map"])
    return reg


def _update(reg, w, how):
    st = w["st"].copy()
    reg.scan_upload(w["scan"])
    if how == "update":
        reg.downsample_skip()
        rep = reg.iekf_update(st, w["st"].copy(), max_iterations=4, imu_en=False)
    else:
        rep = reg.scan_register(st, w["st"].copy(), leaf=0.0, max_iterations=4, imu_en=False)
    return st.pod.copy(), rep


def _apart(a, b):
    """(position difference / 1e-6 m, rotation difference / 1e-7), the larger of the two."""
    return max(np.abs(a[9:12] - b[9:12]).max() / 1e-6, np.abs(a[0:9] - b[0:9]).max() / 1e-7)


@pytest.mark.parametrize("how", ["update", "register"])
def test_the_resident_loop_against_the_host_driven_loop(hall_world, how):
    """lii_iekf_update and lii_scan_register under model 1: the device-resident loop and LII_TEST=host_solve (lii_iekf_iterate driven from
    the host) run the same schedule and end within 1e-6 m / 1e-7 of each other - and more than that away from where model 0 ends."""
    w = hall_world
    out = {}
    for name, env, model in (("device", None, 1), ("host", "host_solve", 1), ("model 0", None, 0)):
        reg = _hall_registrar(w, env)
        try:
            if model:
                reg.set_point_noise()
            out[name] = _update(reg, w, how)
            if model:
                sq = reg.point_noise_download()
                assert int((sq != 0).sum()) == out[name][1]["effect_num"] and sq[sq != 0].max() < EFFECT_CONSTANT
        finally:
            reg.close()
    (sd, rd), (sh, rh), (s0, r0) = out["device"], out["host"], out["model 0"]
    assert (rd["iterations"], rd["searches"], rd["effect_num"]) == (rh["iterations"], rh["searches"], rh["effect_num"])
    assert rd["effect_num"] > 500
    print(f"\n[{how}] device loop against host-driven loop: {_apart(sd, sh):.3f} of the bound; model 1 against model 0: {_apart(sd, s0):.1f} x the bound")
    assert _apart(sd, sh) <= 1.0
    assert _apart(sd, s0) > 1.0, "the weights did not move the result: the comparison above shows nothing"


def _effect_words(reg):
    import lidar_imu_init_amd as lii
    return np.ascontiguousarray(reg.publish_wire_fetch(lii.api.PUB_EFFECT)).view(np.uint32).reshape(-1, 12)


def test_off_means_untouched(cs, refs, hall_world):
    """Model 1, a pass, model 0, the same pass: the 91 doubles are the bytes of a handle that never had the model; the wire effect cloud's
    intensity is the constant again."""
    import lidar_imu_init_amd as lii
    c = refs[SUM_CFG]
    picks = _sum_picks(c, 700, 7100)
    outs = []
    for had_model in (True, False):
        reg = _cluster_registrar(cs, 2048)
        try:
            if had_model:
                reg.set_point_noise()
                d1 = run_scan(reg, c["body"][picks], c["pod"], c["pod2"], SUM_CFG[1])
                reg.clear_point_noise()
                assert reg.point_noise()["model"] == 0 and _code(reg.point_noise_download) == STATE
            d = run_scan(reg, c["body"][picks], c["pod"], c["pod2"], SUM_CFG[1], noise=False)
            outs.append(d)
        finally:
            reg.close()
    assert outs[0]["out"].tobytes() == outs[1]["out"].tobytes() and outs[0]["out2"].tobytes() == outs[1]["out2"].tobytes()
    assert d1["out"][90] == outs[0]["out"][90] and not np.array_equal(d1["out"][:90], outs[0]["out"][:90])
    # the effect cloud
    w = hall_world
    reg = _hall_registrar(w)
    try:
        reg.publish_wire_set(lii.api.PUB_EFFECT, to_host=True)
        reg.set_point_noise()
        _, rep1 = _update(reg, w, "register")
        words1 = _effect_words(reg)
        reg.clear_point_noise()
        s0, rep0 = _update(reg, w, "register")
        words0 = _effect_words(reg)
        assert len(words1) == rep1["effect_num"] and len(words0) == rep0["effect_num"] > 500
        assert np.all(words0[:, 8] == EFFECT_CONSTANT.view(np.uint32)) and not np.any(words1[:, 8] == EFFECT_CONSTANT.view(np.uint32))
    finally:
        reg.close()
    fresh = _hall_registrar(w)
    try:
        s_fresh, _ = _update(fresh, w, "register")
    finally:
        fresh.close()
    assert s0.tobytes() == s_fresh.tobytes()


def test_effect_cloud_carries_the_weights(hall_world):
    """LII_PUB_EFFECT as message bytes under model 1: word 8 of record k is the k-th non-zero entry of the noise buffer, bit for bit; as
    many records as effect_num.  The float4 form keeps refusing an intensity."""
    import lidar_imu_init_amd as lii
    w = hall_world
    reg = _hall_registrar(w)
    try:
        reg.set_point_noise()
        reg.publish_wire_set(lii.api.PUB_EFFECT | lii.api.PUB_DOWN, to_host=True)
        for how in ("register", "update"):
            _, rep = _update(reg, w, how)
            words = _effect_words(reg)
            sq = reg.point_noise_download()
            live = sq[sq != 0]
            assert len(words) == rep["effect_num"] == len(live) > 500
            assert np.array_equal(words[:, 8], live.view(np.uint32)), how
            assert len(np.unique(live)) > 100  # (weights of their own, not one constant)
        reg.publish_set(lii.api.PUB_EFFECT | lii.api.PUB_DOWN | lii.api.PUB_INTENSITY, to_host=True)
        _update(reg, w, "register")
        assert _code(reg.publish_fetch_intensity, lii.api.PUB_EFFECT) == INVALID
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals(cs):
    from lidar_imu_init_amd import api
    reg = _cluster_registrar(cs, 64)
    try:
        L, h = reg.L, reg.h
        good = dict(struct_size=C.sizeof(api.lii_point_noise), model=1, range_inc=0.02, degree_inc=0.05)
        for bad in (dict(struct_size=16), dict(struct_size=32), dict(model=2), dict(model=-1), dict(range_inc=-0.01), dict(degree_inc=-1.0),
                    dict(range_inc=float("nan")), dict(degree_inc=float("inf")), dict(model=0, range_inc=float("nan"))):
            f = {**good, **bad}
            m = api.lii_point_noise(f["struct_size"], f["model"], f["range_inc"], f["degree_inc"])
            assert L.lii_point_noise_set(h, C.byref(m)) == INVALID, bad
        assert reg.point_noise() == dict(model=0, range_inc=0.0, degree_inc=0.0)
        m = api.lii_point_noise(8, 0, 0.0, 0.0)
        assert L.lii_point_noise_get(h, C.byref(m)) == INVALID and L.lii_point_noise_get(h, None) == INVALID
        n = C.c_int32(-1)
        buf = np.zeros(64, np.float32)
        fp = buf.ctypes.data_as(C.POINTER(C.c_float))
        assert L.lii_point_noise_download(h, fp, 64, None) == INVALID
        assert L.lii_point_noise_download(h, fp, 64, C.byref(n)) == STATE     # model 0
        reg.set_point_noise(0.03, 0.1)
        assert reg.point_noise() == dict(model=1, range_inc=0.03, degree_inc=0.1)
        assert L.lii_point_noise_download(h, fp, 64, C.byref(n)) == STATE     # no pass since the model was set
        import lidar_imu_init_amd as lii
        bodies = cs.filler_bodies("identity", 8)
        reg.scan_upload(pr.scan_of(bodies))
        reg.downsample_skip()
        reg.iekf_iterate(lii.State(pr.POSES["identity"].pod(lii.State().pod)), True, False)
        assert L.lii_point_noise_download(h, fp, 7, C.byref(n)) == CAPACITY and n.value == 8
        assert L.lii_point_noise_download(h, fp, 8, C.byref(n)) == 0 and n.value == 8 and not buf.any()
        reg.set_point_noise(0.03, 0.1)                                        # set again: the buffer is the next pass's
        assert L.lii_point_noise_download(h, fp, 8, C.byref(n)) == STATE
    finally:
        reg.close()
    # a communicator attached; and lii_comm_init on a handle with model 1
    reg = _cluster_registrar(cs, 64)
    try:
        reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")
        assert _code(reg.set_point_noise) == STATE and _code(reg.clear_point_noise) == STATE
        assert reg.point_noise()["model"] == 0
    finally:
        reg.close()
    reg = _cluster_registrar(cs, 64)
    try:
        reg.set_point_noise()
        assert _code(reg.comm_init, 1, 0, reg.comm_unique_id(), "rccl") == STATE
        assert reg.point_noise()["model"] == 1 and reg.comm_describe() == "no communicator"
        reg.clear_point_noise()
        reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")  # model 0: a communicator attaches as ever
    finally:
        reg.close()
