"""lii_pose_score / lii_pose_score_dev on the device: the figures of one search pass at K candidate poses, against the oracle's pass at
each pose, and the rules of the call - pose k's bits do not depend on its batch, the handle's registration state is left alone, bad
members of a batch score zeros, argument and state errors, the in-place map.

Hall map of small_world, the `tiny` scan (2 048 points) through scan_upload + downsample_skip (tests/pose_score_cases.py).
Where the kernel changes path: a workgroup holds 64 consecutive points of one pose (n_down = 2 000 leaves the last one 16), the final
pass sums four poses per workgroup (K = 4, 5), the host form stages chunks of 2^22 / n_down poses (K = 2 049 at 2 048 points), and a
launch of up to 2 048 workgroups searches with four wavefronts per workgroup, a larger one with one (32 workgroups per pose at 2 048
points: K = 64 is the last of the first kind, K = 65 the first of the second - a pose scored alone is held to its bits in either).
"""
import ctypes as C

import numpy as np
import pytest

import pose_score_cases as psc
from plane_rows_np import _ulp32  # pd2's allowance: one float32 ulp of the value

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5  # LII_ERR_INVALID, LII_ERR_STATE


def _code(f):
    import lidar_imu_init_amd as lii
    try:
        f()
        return 0
    except lii.LIIError as e:
        return e.code


@pytest.fixture(scope="module")
def world(oracle, small_world):
    import lidar_imu_init_amd as lii
    _, map_pts = small_world
    reg = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    tree = oracle.Tree("oracle")
    tree.build(map_pts)
    yield dict(reg=reg, tree=tree, scan=psc.tiny_scan(small_world))
    reg.close()


def _load(reg, scan):
    reg.scan_upload(scan)
    assert reg.downsample_skip() == len(scan)


def _base(oracle, r_li=None, t_li=None):
    import lidar_imu_init_amd as lii
    return lii.State(psc.state_at(oracle, psc.TRUE_R, psc.TRUE_P, r_li, t_li))


def _pool(small_world, K):
    """K distinct good poses: the 23 of the parity set's first batch, repeated with the position moved 1 cm in x per round."""
    _, _, R, p = psc.parity_poses(small_world)[0]
    idx = np.arange(K) % len(R)
    return R[idx].copy(), p[idx] + np.c_[0.01 * (np.arange(K) // len(R)), np.zeros(K), np.zeros(K)]


def _score_bytes(out, k):
    n_full, eff, tot, res = out
    return (int(n_full[k]), int(eff[k]), np.float64(tot[k]).tobytes(), res[k].tobytes())


def test_oracle_parity(world, oracle, small_world):
    import lidar_imu_init_amd as lii
    reg, tree, scan = world["reg"], world["tree"], world["scan"]
    _load(reg, scan)
    n = len(scan)
    assert n == 2048
    flips_all, pairs_all, K_all, short_lists = 0, 0, 0, []
    for r_li, t_li, R, p in psc.parity_poses(small_world):
        base = lii.State(psc.state_at(oracle, R[0], p[0], r_li, t_li))
        n_full, eff, tot, res = reg.pose_score(base, (R, p), want_res=True)
        assert res.shape == (len(R), n)
        for k in range(len(R)):
            ref = tree.iterate_once(scan, psc.state_at(oracle, R[k], p[k], r_li, t_li), search=True, imu_en=False, threads=4)
            assert n_full[k] == int((ref["nearest_n"] == 5).sum())
            short_lists.append(n - int(n_full[k]))
            sel, ref_sel = res[k] >= 0, ref["selected"].astype(bool)
            flips = int((sel != ref_sel).sum())
            print(f"pose {K_all + k}: n_full {n_full[k]} effect {eff[k]} (oracle {int(ref_sel.sum())}) flags that differ {flips} total_residual {tot[k]:.6f}")
            assert flips <= 0.001 * n
            flips_all += flips
            pairs_all += n
            both = sel & ref_sel
            want = np.abs(ref["normvec"][both, 3])
            tol = np.array([_ulp32(v) for v in want]) if both.any() else np.zeros(0)
            assert np.all(np.abs(res[k][both].astype(np.float64) - want.astype(np.float64)) <= tol)
            assert np.all(res[k][~sel] == np.float32(-1000.0))
            assert eff[k] == int(sel.sum())
            s = float(res[k][sel].astype(np.float64).sum())
            assert abs(tot[k] - s) <= n * 2.0 ** -52 * tot[k]
            if not sel.any():
                assert tot[k] == 0.0
        K_all += len(R)
    assert K_all == 24
    print(f"batch: {flips_all} flags differ of {pairs_all}")
    assert flips_all <= 0.001 * pairs_all
    # the cases are what they claim: the true pose selects nearly everything, the far-off guess little, and the pose at the wall leaves
    # many lists short (queries past the map's edge)
    assert short_lists[0] < 0.01 * n and short_lists[3] > 0.1 * n


@pytest.mark.parametrize("n_down", [2048, 2000])
def test_batch_independence_and_repeatability(world, oracle, small_world, n_down):
    reg, scan = world["reg"], world["scan"][:n_down]
    _load(reg, scan)
    base = _base(oracle)
    _, _, R, p = psc.parity_poses(small_world)[0]
    targets = (0, 2, 3)  # the true pose, the far-off guess, the pose at the wall
    alone = {}
    for t in targets:
        a = reg.pose_score(base, (R[t:t + 1], p[t:t + 1]), want_res=True)
        b = reg.pose_score(base, (R[t:t + 1], p[t:t + 1]), want_res=True)
        alone[t] = _score_bytes(a, 0)
        assert alone[t] == _score_bytes(b, 0)
        assert a[1][0] == int((a[3][0] >= 0).sum())
    Ks = (1, 2, 4, 5, 63, 64, 65, 257) + ((2049,) if n_down == 2048 else ())
    for K in Ks:
        fR, fp = _pool(small_world, K)
        for t in targets if K < 2049 else targets[:1]:
            A_R, A_p = fR.copy(), fp.copy()
            A_R[0], A_p[0] = R[t], p[t]
            B_R, B_p = fR[::-1].copy(), fp[::-1].copy()
            B_R[K - 1], B_p[K - 1] = R[t], p[t]
            assert _score_bytes(reg.pose_score(base, (A_R, A_p), want_res=True), 0) == alone[t], (K, t, "first")
            assert _score_bytes(reg.pose_score(base, (B_R, B_p), want_res=True), K - 1) == alone[t], (K, t, "last")
    # without res the scores are the same bits
    fR, fp = _pool(small_world, 65)
    with_res = reg.pose_score(base, (fR, fp), want_res=True)
    without = reg.pose_score(base, (fR, fp))
    assert all(np.array_equal(x, y) for x, y in zip(with_res[:3], without)) and np.array_equal(with_res[2].view(np.uint64), without[2].view(np.uint64))


def test_leaves_the_handle_alone(world, oracle, small_world):
    import lidar_imu_init_amd as lii
    reg, scan = world["reg"], world["scan"]
    n = len(scan)
    Rw, pw = psc.perturbed(False)
    st = psc.state_at(oracle, Rw, pw)
    st2 = oracle.state_boxplus(st, np.r_[0.001, -0.002, 0.0015, 0.01, -0.005, 0.004, np.zeros(18)])
    fR, fp = _pool(small_world, 64)

    def run(score):
        _load(reg, scan)
        out1 = reg.iekf_iterate(lii.State(st), True, False)
        unfinished = reg.last_unfinished_queries()
        if score:
            reg.pose_score(lii.State(st2), (fR, fp), want_res=True)
            assert reg.last_unfinished_queries() == unfinished
        out2 = reg.iekf_iterate(lii.State(st2), False, False)
        nb, cnt, sel = reg.neighbors(n)
        return out1, out2, nb, cnt, sel, unfinished

    plain, scored = run(False), run(True)
    assert np.array_equal(plain[0].view(np.uint64), scored[0].view(np.uint64))
    assert np.array_equal(plain[1].view(np.uint64), scored[1].view(np.uint64)), "all 91 sums of the pass on cached planes"
    assert np.array_equal(plain[2].view(np.uint32), scored[2].view(np.uint32)) and np.array_equal(plain[3], scored[3])
    assert np.array_equal(plain[4], scored[4]) and plain[5] == scored[5]
    assert int(plain[1][90]) > 0.9 * n


def test_bad_members_of_a_batch(world, oracle, small_world):
    reg, scan = world["reg"], world["scan"][:2000]
    _load(reg, scan)
    base = _base(oracle)
    R, p = _pool(small_world, 9)
    good = [_score_bytes(reg.pose_score(base, (R[k:k + 1], p[k:k + 1]), want_res=True), 0) for k in range(9)]
    bad = (1, 4, 8)
    R[1, 1, 2] = np.nan           # a NaN entry of the rotation
    p[4, 0] = np.inf              # an Inf position
    p[8] = [10_000.0, 0.0, 0.0]   # 10 km away: every point finds nothing within reach
    out = reg.pose_score(base, (R, p), want_res=True)
    for k in range(9):
        if k in bad:
            assert (int(out[0][k]), int(out[1][k]), float(out[2][k])) == (0, 0, 0.0)
            assert np.all(out[3][k] == np.float32(-1000.0))
        else:
            assert _score_bytes(out, k) == good[k]
    # every point outside the ADDRESSABLE grid (2^20 cells of 0.3 m to either side) scores the same zeros
    p[8] = [1.0e6, -1.0e6, 1.0e6]
    out = reg.pose_score(base, (R, p), want_res=True)
    assert (int(out[0][8]), int(out[1][8]), float(out[2][8])) == (0, 0, 0.0) and np.all(out[3][8] == np.float32(-1000.0))
    assert _score_bytes(out, 0) == good[0] and _score_bytes(out, 7) == good[7]


def _dev_array(reg, addr, shape, dtype):
    """device memory -> numpy, through the runtime the library itself uses"""
    hip = C.CDLL(reg.L._name)
    out = np.zeros(shape, dtype)
    reg.synchronize()
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(int(addr)), C.c_size_t(out.nbytes), C.c_int(2)) == 0  # hipMemcpyDeviceToHost
    return out


def test_argument_and_state_errors_and_the_device_form(world, oracle, small_world):
    import lidar_imu_init_amd as lii
    from lidar_imu_init_amd.api import POSE_SCORE_DTYPE, poses_array
    reg, scan = world["reg"], world["scan"][:2000]
    _load(reg, scan)
    n = len(scan)
    base = _base(oracle)
    K = 65
    P = poses_array(_pool(small_world, K))
    L, h = reg.L, reg.h
    sc = np.zeros(K, POSE_SCORE_DTYPE)
    res = np.zeros((K, n), np.float32)
    d_P, d_sc, d_res = reg.dev_alloc(P.nbytes), reg.dev_alloc(sc.nbytes), reg.dev_alloc(res.nbytes)
    reg.dev_upload(d_P, P)

    def both(base_p=True, poses=True, k=K, scores=True):
        rc_h = L.lii_pose_score(h, base.pod.ctypes.data if base_p else None, P.ctypes.data if poses else None, k, sc.ctypes.data if scores else None, res.ctypes.data)
        rc_d = L.lii_pose_score_dev(h, base.pod.ctypes.data if base_p else None, d_P if poses else None, k, d_sc if scores else None, d_res)
        return rc_h, rc_d

    # LII_ERR_INVALID: NULL arguments, n_poses < 1 or > 65 536
    assert L.lii_pose_score(None, base.pod.ctypes.data, P.ctypes.data, K, sc.ctypes.data, None) == INVALID
    assert L.lii_pose_score_dev(None, base.pod.ctypes.data, d_P, K, d_sc, None) == INVALID
    assert both(base_p=False) == (INVALID, INVALID)
    assert both(poses=False) == (INVALID, INVALID)
    assert both(scores=False) == (INVALID, INVALID)
    assert both(k=0) == (INVALID, INVALID) and both(k=-3) == (INVALID, INVALID) and both(k=65_537) == (INVALID, INVALID)
    # the device form gives the host form's bytes (this cloud keeps its order on the device: downsample_skip)
    assert both() == (0, 0)
    assert np.array_equal(_dev_array(reg, d_sc, (K,), POSE_SCORE_DTYPE).view(np.uint8), sc.view(np.uint8))
    assert np.array_equal(_dev_array(reg, d_res, (K, n), np.float32).view(np.uint32), res.view(np.uint32))
    assert (sc["effect_num"] > 0).all()
    # ... and res may be left out in both
    sc2 = np.zeros(K, POSE_SCORE_DTYPE)
    assert L.lii_pose_score(h, base.pod.ctypes.data, P.ctypes.data, K, sc2.ctypes.data, None) == 0 and np.array_equal(sc2.view(np.uint8), sc.view(np.uint8))
    reg.dev_upload(d_sc, np.zeros(K, POSE_SCORE_DTYPE))
    assert L.lii_pose_score_dev(h, base.pod.ctypes.data, d_P, K, d_sc, None) == 0
    assert np.array_equal(_dev_array(reg, d_sc, (K,), POSE_SCORE_DTYPE).view(np.uint8), sc.view(np.uint8))
    # LII_ERR_INVALID: n_poses * n_down >= 2^31 (a cloud of 32 768 points x 65 536 poses)
    big = lii.Registrar(max_scan_points=40_000, max_map_points=400_000, filter_size_map=0.15)
    big.map_build(small_world[1])
    cloud = np.zeros((32_768, 4), np.float32)
    cloud[:, :3] = np.tile(world["scan"][:, :3], (16, 1))
    _load(big, cloud)
    Pb = np.zeros((65_536, 12))
    scb = np.zeros(65_536, POSE_SCORE_DTYPE)
    assert big.L.lii_pose_score(big.h, base.pod.ctypes.data, Pb.ctypes.data, 65_536, scb.ctypes.data, None) == INVALID
    assert big.L.lii_pose_score_dev(big.h, base.pod.ctypes.data, d_P, 65_536, d_sc, None) == INVALID  # (refused before any pointer is used)
    big.close()
    # LII_ERR_STATE: no down-sampled cloud; no map
    r2 = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    assert _code(lambda: r2.pose_score(base, P)) == STATE  # neither
    r2.map_build(small_world[1])
    assert _code(lambda: r2.pose_score(base, P)) == STATE  # a map, no cloud
    r2.close()
    r3 = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    _load(r3, scan)
    assert _code(lambda: r3.pose_score(base, P)) == STATE  # a cloud, no map
    d3 = [r3.dev_alloc(P.nbytes), r3.dev_alloc(sc.nbytes)]
    assert r3.L.lii_pose_score_dev(r3.h, base.pod.ctypes.data, d3[0], K, d3[1], None) == STATE
    # LII_ERR_STATE: from inside lii_scan_job::while_waiting
    r3.map_build(small_world[1])
    seen = []
    st = lii.State(psc.state_at(oracle, *psc.perturbed(False)))
    r3.scan_upload(scan)
    r3.scan_register(st, st.copy(), leaf=0.0, max_iterations=2,
                     while_waiting=lambda: seen.append((_code(lambda: r3.pose_score(base, P)),
                                                        r3.L.lii_pose_score_dev(r3.h, base.pod.ctypes.data, d3[0], K, d3[1], None))))
    assert seen == [(STATE, STATE)]
    assert _code(lambda: r3.pose_score(base, P)) == 0  # ... and behind the call it is served again
    r3.close()


def test_in_place_map_not_committed(oracle, small_world):
    """A map_add_points batch that nobody has committed: the call passes through commit_map and scores the map WITH the batch, as the
    oracle tree does after the same add_points."""
    import lidar_imu_init_amd as lii
    _, map_pts = small_world
    scan = psc.tiny_scan(small_world)
    # the map without the hall's +x half of the floor and walls, the rest added in place
    late = map_pts[:, 0] > 2.0
    first, batch = map_pts[~late], map_pts[late]
    reg = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(first)
    tree = oracle.Tree("oracle", downsample=0.15)
    tree.build(first)
    _load(reg, scan)
    n = len(scan)
    _, _, R, p = psc.parity_poses(small_world)[0]
    R, p = R[:4], p[:4]
    base = lii.State(psc.state_at(oracle, R[0], p[0]))
    before = reg.pose_score(base, (R, p))
    reg.map_add_points(batch, False)
    tree.add_points(batch, False)
    n_full, eff, tot, res = reg.pose_score(base, (R, p), want_res=True)
    assert n_full[0] > before[0][0] and eff[0] > before[1][0]  # the batch is in
    for k in range(4):
        ref = tree.iterate_once(scan, psc.state_at(oracle, R[k], p[k]), search=True, imu_en=False, threads=4)
        assert n_full[k] == int((ref["nearest_n"] == 5).sum())
        sel, ref_sel = res[k] >= 0, ref["selected"].astype(bool)
        assert int((sel != ref_sel).sum()) <= 0.001 * n
        both = sel & ref_sel
        want = np.abs(ref["normvec"][both, 3])
        assert np.all(np.abs(res[k][both].astype(np.float64) - want.astype(np.float64)) <= np.array([_ulp32(v) for v in want]))
        assert eff[k] == int(sel.sum())
        assert abs(tot[k] - float(res[k][sel].astype(np.float64).sum())) <= n * 2.0 ** -52 * tot[k]
    reg.close()
