"""Every k-NN completion path of lii_fit.hip against the CPU tree, brute force and (where it is built) the reference's own tree.

A search pass leaves the queries it cannot prove exact to the completion (knn_fallback_wave); which code finishes them depends on how many
a pass flags - 1 .. 96: one per completion workgroup, four wavefronts together (complete_one_coop); 97 .. 256: one wavefront each in the
completion workgroups (complete_one); more: every workgroup its own (complete_flagged), or, once two such scans in a row have switched
the launch plan on, k_complete_listed for the first 4096 - and on whether the map has its dense cell window (row trips) or not (column
walk), whether the search pass measured the inner cells (seeded) or not, and how the far list fills.  tests/completion_cases.py builds
inputs for each of these and tests/test_completion_cases_host.py asserts on the CPU that they are what they claim.

Lists are exact by the project's rule (tests/test_gpu_register.py): NO tolerance.  check_lists compares counts for every query and the
lists bit for bit in points and recomputed float32 distances; a query whose reference has d5 == d6 is compared in distances and map
membership only, and outside the tie patches such queries must stay below 1 % of each class.

Measured on the MI355X (lii_last_unfinished_queries): C0 = 0 - the F-queries alone flag nothing - and every scan of tests a and b
reported exactly C0 + U_n, on both map variants and with LII_WIDE_COMPLETION on and off; no query of any class was excluded for a 5/6
tie outside the tie patches.  Two deliberately wrong builds were run against this file: without the `part == 0` condition where the inner
result re-enters knn_fallback_wave, tests a[96], b (scan 11) and d[coop] fail; with kFarCap for kFarUse in far_list_trip's first test,
test d fails on the brim query whose one trip lists kFarUse + 1 chunks.
"""
import numpy as np
import pytest

import completion_cases as cc

pytestmark = pytest.mark.gpu

START_ERROR = np.r_[0.004, -0.003, 0.005, 0.03, -0.02, 0.01, np.zeros(18)]


class MapCase:
    """One map with its CPU references: the restated tree, the reference's tree where it is built, brute force on a fixed sample."""

    def __init__(self, oracle, map_pts, queries, brute_ids, tree=None):
        self.map = map_pts
        self.queries = queries
        self.tree = tree
        if tree is None:
            self.tree = oracle.Tree("oracle")
            self.tree.build(map_pts)
        self.ref_tree = None
        if oracle.ref_available():
            self.ref_tree = oracle.Tree("ref")
            self.ref_tree.build(map_pts)
        self.map_set = cc.point_set(map_pts)
        self.brute_ids = np.asarray(brute_ids)
        self.brute_row = np.full(len(queries), -1)
        self.brute_row[self.brute_ids] = np.arange(len(self.brute_ids))
        self.brute = cc.brute_knn(queries, map_pts, self.brute_ids)


@pytest.fixture(scope="module")
def hole(small_world, oracle):
    hw = cc.HoleWorld(small_world, oracle)
    brute_ids = np.r_[np.arange(0, cc.F_N, 30), cc.F_N + np.arange(cc.BRUTE_SAMPLE)]
    cases = {v: MapCase(oracle, hw.maps[v], hw.queries, brute_ids, tree=hw.tree if v == "win" else None) for v in ("win", "hashed")}
    return hw, cases


@pytest.fixture(scope="module")
def slab(small_world, oracle):
    sw = cc.SlabWorld(small_world, oracle)
    special = np.flatnonzero(sw.group != "F")
    maps = {"win": sw.map, "hashed": np.ascontiguousarray(np.r_[sw.map, cc.FAR_POINTS])}
    assert cc.has_window(maps["win"]) and not cc.has_window(maps["hashed"])
    for p in cc.FAR_POINTS:
        assert cc.dist2_f32(sw.queries, p).min() > 5.0
    cases = {v: MapCase(oracle, maps[v], sw.queries, special, tree=sw.tree if v == "win" else None) for v in ("win", "hashed")}
    return sw, cases


def registrar(map_pts):
    import lidar_imu_init_amd as lii
    reg = lii.Registrar(max_scan_points=16_384, max_map_points=200_000, filter_size_map=cc.FILTER_SIZE_MAP)
    reg.map_build(map_pts)
    assert reg.map_size() == len(map_pts)  # every point is kept, duplicates included
    return reg


def check_lists(reg, case, n, ids, classes, relaxed=None, identity=True):
    """The device lists of the last search launch against every reference.  ids: the scan's query ids; classes: {name: mask over the
    scan}; relaxed: the queries where a 5/6 tie is intended (the tie patches); identity: the scan was searched at identity pose, where
    its world points must be its body points - the brute-force lists computed once per map then apply."""
    # (rb.world is written by the search launch, k_knn_ck, and by a fit launch on cached planes - never by one behind a search launch:
    # after an update whose last pass searched it holds the points the lists were searched for)
    world = np.ascontiguousarray(reg.scan_download(2)[:, :3])
    assert len(world) == n == len(ids)
    nb, cnt, _ = reg.neighbors(n)
    if identity:
        assert np.array_equal(world.view(np.uint32), case.queries[ids].view(np.uint32))
    if relaxed is None:
        relaxed = np.zeros(n, bool)
    shares = {}
    for name, tree in (("tree", case.tree), ("reference tree", case.ref_tree)):
        if tree is None:
            continue
        ref = cc.Reference(tree, world)
        problems = cc.lists_agree(world, nb, cnt, ref.pts, ref.d2, ref.cnt, ref.tie56, case.map_set)
        assert not problems, (name, problems)
        for cname, mask in classes.items():
            excluded = int((ref.tie56 & mask & ~relaxed).sum())
            shares[(name, cname)] = (excluded, int(mask.sum()))
            assert excluded <= 0.01 * mask.sum(), (name, cname, excluded, int(mask.sum()))
    # brute force on the fixed sample
    pos = np.flatnonzero(case.brute_row[ids] >= 0)
    if identity:
        rows = case.brute_row[ids[pos]]
        bp, bd, bc = (a[rows] for a in case.brute)
    else:
        bp, bd, bc = cc.brute_knn(world, case.map, pos)
    tie = (bc >= 6) & (bd[:, 4] == bd[:, 5])
    problems = cc.lists_agree(world[pos], nb[pos], cnt[pos], np.ascontiguousarray(bp[:, :5]), bd, np.minimum(bc, 5).astype(np.int32), tie, case.map_set)
    assert not problems, ("brute force", problems)
    assert (tie & ~relaxed[pos]).sum() <= 0.01 * max(len(pos), 100)
    print("    queries excluded for a 5/6 tie (excluded, of):", shares, "brute-force sample:", len(pos))


def hole_classes(ids):
    return {"F": ids < cc.F_N, "U": ids >= cc.F_N}


# ------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("variant", ["win", "hashed"])
@pytest.mark.parametrize("u_n", cc.U_EDGES)
def test_host_driven_pass_every_capacity_edge(hole, variant, u_n):
    """lii_iekf_iterate: 1 - 96 flagged queries go to complete_one_coop, 97 - 256 to complete_one in the completion workgroups, more to
    complete_flagged in every workgroup of the cloud (the host-driven pass has no launch plan)."""
    import lidar_imu_init_amd as lii
    hw, cases = hole
    case = cases[variant]
    scan, ids = hw.scan(u_n)
    reg = registrar(case.map)
    try:
        reg.scan_upload(scan)
        n = reg.downsample_skip()
        assert n == len(scan)
        reg.iekf_iterate(lii.State(), True, False)
        unfinished = reg.last_unfinished_queries()
        print(f"\n[a {variant}] U_n = {u_n}: unfinished {unfinished}, intended {cc.C0 + u_n}")
        assert unfinished == cc.C0 + u_n
        check_lists(reg, case, n, ids, hole_classes(ids))
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize("variant", ["win", "hashed"])
@pytest.mark.parametrize("wide", [True, False])
def test_scan_register_with_the_launch_plan(hole, monkeypatch, variant, wide):
    """lii_scan_register, one search pass per scan: scans 3 - 5 run with k_complete_listed enqueued (over and under kListCap), scans 6 and 7
    with it enqueued and nothing to do, scan 9 is the single outlier with the plan off, scans 10 and 11 stand on either side of the
    completion workgroups' one-query capacity.  LII_WIDE_COMPLETION=0 (every workgroup its own, always) is held to the same references."""
    import lidar_imu_init_amd as lii
    hw, cases = hole
    case = cases[variant]
    monkeypatch.setenv("LII_WIDE_COMPLETION", "1" if wide else "0")  # (read when the handle is created)
    reg = registrar(case.map)
    try:
        for k, u_n in enumerate(cc.PLAN_SEQUENCE):
            scan, ids = hw.scan(u_n)
            reg.scan_upload(scan)
            rep = reg.scan_register(lii.State(), lii.State(), leaf=0.0, max_iterations=1, imu_en=False)
            assert rep["searches"] == 1 and rep["iterations"] == 1
            unfinished = reg.last_unfinished_queries()
            print(f"\n[b {variant} wide={int(wide)}] scan {k + 1}, U_n = {u_n}: unfinished {unfinished}, intended {cc.C0 + u_n}")
            assert unfinished == cc.C0 + u_n
            check_lists(reg, case, len(scan), ids, hole_classes(ids))
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------ c
@pytest.mark.parametrize("variant", ["win", "hashed"])
@pytest.mark.parametrize("u_n", [6000, 1500])
def test_whole_update_in_the_wide_regime(hole, oracle, monkeypatch, variant, u_n):
    """The iterated update (four passes, two of them searching) on the third of three wide scans - its search launches are followed by
    k_complete_listed - against the oracle's update, then the lists of its last search pass."""
    import lidar_imu_init_amd as lii
    hw, cases = hole
    case = cases[variant]
    monkeypatch.setenv("LII_WIDE_COMPLETION", "1")
    scan, ids = hw.scan(u_n)
    st0 = oracle.state_boxplus(oracle.state_init(), START_ERROR)
    ref = case.tree.iekf_update(scan, st0, st0, max_iterations=4, imu_en=False, threads=4)
    # (the lists the device holds afterwards are those of its last search pass, rb.world those of its last pass: the same pass here)
    assert ref["logs"][-1, 0] == 1
    reg = registrar(case.map)
    try:
        for _ in range(2):
            reg.scan_upload(scan)
            reg.scan_register(lii.State(), lii.State(), leaf=0.0, max_iterations=1, imu_en=False)
            assert reg.last_unfinished_queries() > cc.K_FLAG_CAP
        reg.scan_upload(scan)
        s = lii.State(st0)
        rep = reg.scan_register(s, lii.State(st0), leaf=0.0, max_iterations=4, imu_en=False)
        print(f"\n[c {variant}] U_n = {u_n}: iterations {rep['iterations']}, searches {rep['searches']}, unfinished {reg.last_unfinished_queries()}")
        assert rep["iterations"] == ref["iters"]
        v = oracle.StateView(ref["state"])
        dp = np.linalg.norm(v.pos_end - s.pos_end)
        dth = np.linalg.norm(oracle.log_so3(v.rot_end.T @ s.rot_end))
        print(f"    |dp| = {dp:.3e} m, |dtheta| = {dth:.3e} rad")
        assert dp <= 1e-6 and dth <= 1e-7
        check_lists(reg, case, len(scan), ids, hole_classes(ids), identity=False)
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------ d
@pytest.mark.parametrize("variant", ["win", "hashed"])
@pytest.mark.parametrize("mix", list(cc.SLAB_MIXES))
def test_far_list_overflow_and_unseeded_completions(slab, monkeypatch, variant, mix):
    """The slab map: queries facing a slab dense enough that single trips of the far pass exceed the far list (lane by lane) and the ball
    lists three lists' worth, queries facing one whose trips fit and fill the list (scanned and reset), two whose one trip lists exactly
    kFarUse and kFarUse + 1 chunks with the nearest point last, queries inside a slab (the search pass's table overflows: unseeded)
    and in front of wall patches present two and four times (ties; four copies: ambiguous, unseeded with a small ball) - through the
    host-driven pass and through the third of three lii_scan_register calls, brute force on all of them."""
    import lidar_imu_init_amd as lii
    sw, cases = slab
    case = cases[variant]
    scan, ids, lo, hi = sw.scan(mix)
    group = sw.group[ids]
    classes = {name: group == name for name in ("F", "U", "facing_a", "facing_b", "in_slab", "brim")}
    relaxed = group == "tie"
    assert cc.SLAB_MIX_RANGE[mix][0] <= lo and hi <= cc.SLAB_MIX_RANGE[mix][1]
    monkeypatch.setenv("LII_WIDE_COMPLETION", "1")
    reg = registrar(case.map)
    try:
        reg.scan_upload(scan)
        n = reg.downsample_skip()
        assert n == len(scan)
        reg.iekf_iterate(lii.State(), True, False)
        unfinished = reg.last_unfinished_queries()
        print(f"\n[d {variant} {mix}] host-driven pass: unfinished {unfinished} (sure {lo}, at most {hi})")
        assert lo <= unfinished <= hi
        check_lists(reg, case, n, ids, classes, relaxed)
        for _ in range(3):
            reg.scan_upload(scan)
            rep = reg.scan_register(lii.State(), lii.State(), leaf=0.0, max_iterations=1, imu_en=False)
            assert rep["searches"] == 1
            assert reg.last_unfinished_queries() == unfinished
        check_lists(reg, case, n, ids, classes, relaxed)
    finally:
        reg.close()


# ------------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize("variant", ["win", "hashed"])
def test_listed_completion_is_deterministic(hole, monkeypatch, variant):
    """Scan 3 of test b (more flagged queries than the list holds, k_complete_listed enqueued) on two fresh handles: the same bytes."""
    import lidar_imu_init_amd as lii
    hw, cases = hole
    monkeypatch.setenv("LII_WIDE_COMPLETION", "1")
    scan, _ = hw.scan(cc.PLAN_SEQUENCE[2])
    got = []
    for _ in range(2):
        reg = registrar(cases[variant].map)
        try:
            for _ in range(3):
                reg.scan_upload(scan)
                reg.scan_register(lii.State(), lii.State(), leaf=0.0, max_iterations=1, imu_en=False)
            nb, cnt, _ = reg.neighbors(len(scan))
            got.append((nb.tobytes(), cnt.tobytes()))
        finally:
            reg.close()
    assert got[0] == got[1]
