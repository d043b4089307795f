"""Preconditions of tests/test_gpu_completion_paths.py, asserted on the CPU: the inputs of tests/completion_cases.py are what that
module says they are - class sizes, the window arithmetic, the chunk sums of the slab-facing queries, the tie share - and its brute
force agrees with the CPU trees bit for bit."""
import os
import re

import numpy as np
import pytest

import completion_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_imu_init_amd", "csrc")


@pytest.fixture(scope="module")
def hole(small_world, oracle):
    return cc.HoleWorld(small_world, oracle)


@pytest.fixture(scope="module")
def slab(small_world, oracle):
    return cc.SlabWorld(small_world, oracle)


def _const(text, name):
    return int(re.search(r"constexpr int " + name + r"\s*=\s*(\d+)\s*;", text).group(1))


def test_capacities_are_the_sources():
    dev = open(os.path.join(CSRC, "lii_device.h")).read()
    fit = open(os.path.join(CSRC, "lii_fit.hip")).read()
    knn = open(os.path.join(CSRC, "lii_knn.hip")).read()
    mapc = open(os.path.join(CSRC, "lii_capi_map.cpp")).read()
    assert _const(dev, "kFlagCap") == cc.K_FLAG_CAP
    assert _const(dev, "kListCap") == cc.K_LIST_CAP
    assert _const(dev, "kCompletionBlocksPre") == cc.K_COMPLETION_BLOCKS_PRE
    assert _const(fit, "kFarCap") == cc.K_FAR_CAP and "kFarUse = kFarCap - 1" in fit
    # the search pass's table: MAXCH = 1 << kChunkBits chunks of LPQ = 4 points (k_knn_ck<4, ...>)
    assert 1 << _const(knn, "kChunkBits") == cc.SEARCH_TABLE_CHUNKS and "k_knn_ck<4," in knn
    assert "(64u << 20)" in mapc and cc.WINDOW_BYTES == 64 << 20
    assert set(cc.U_EDGES) == {0, 1, 96, 97, 256, 257, 1500, 4096, 4097, 6000}


def test_class_sizes(hole):
    assert len(hole.maps["win"]) == 64896
    assert len(hole.F) == cc.F_N and len(hole.U) == cc.U_MAX
    assert hole.f_ok.sum() == len(hole.f_ok)  # every random floor point outside the hole is sure-finished
    assert len(np.unique(hole.queries, axis=0)) == len(hole.queries)
    # no genuine 5/6 tie among them
    assert hole.f_ref_all.tie56.sum() == 0 and hole.u_ref_all.tie56.sum() == 0
    for u_n in cc.U_EDGES:
        scan, ids = hole.scan(u_n)
        assert scan.shape == (cc.F_N + u_n, 4) and hole.is_U(ids).sum() == u_n and len(scan) <= 9000
        assert np.array_equal(scan[:, :3], hole.queries[ids]) and not scan[:, 3].any()


def test_window_and_no_window_arithmetic(hole):
    entries, dims = cc.window_entries(hole.maps["win"])
    # 24 x 18 x 6 m at 0.45 m cells: blocks -4..3, -3..2, -1..1 and a block of margin on every side
    assert dims == [80, 64, 40] and entries * 8 <= cc.WINDOW_BYTES and cc.has_window(hole.maps["win"])
    entries, dims = cc.window_entries(hole.maps["hashed"])
    assert dims == [288, 288, 288] and entries * 8 > cc.WINDOW_BYTES and not cc.has_window(hole.maps["hashed"])
    # the two far points are out of every query's reach
    for p in cc.FAR_POINTS:
        assert cc.dist2_f32(hole.queries, p).min() > 5.0


def test_slab_chunk_sums(slab):
    assert len(slab.map) <= 200_000
    keys, counts = slab.cell_counts()
    layer0 = (keys[:, 0] == cc.SLAB_A_X[0]) & (keys[:, 1] >= cc.SLAB_A_Y[0]) & (keys[:, 1] <= cc.SLAB_A_Y[1]) & (keys[:, 2] >= cc.SLAB_A_Z[0]) & (keys[:, 2] <= cc.SLAB_A_Z[1])
    assert layer0.sum() >= 11 * 11 and counts[layer0].min() >= 80
    assert cc.has_window(slab.map)
    assert len(slab.facing_a) >= 64 and len(slab.facing_b) >= 64
    for q in slab.facing_a:
        assert (cc.dist2_f32(slab.map, q) <= 0.81).sum() < 5
        d_face = cc.SLAB_A_X[0] * float(cc.CELL) - q[0]
        assert 1.0 <= d_face <= 2.0
        assert slab.ball_chunks(q, keys, counts) >= 3 * cc.K_FAR_USE
        assert max(slab.row_trip_totals(q)) > cc.K_FAR_USE      # a single trip too large for the list: lane by lane
    for q in slab.facing_b:
        assert (cc.dist2_f32(slab.map, q) <= 0.81).sum() < 5
        trips = slab.row_trip_totals(q)
        assert max(trips) <= 64 * ((cc.SLAB_B + 3) // 4) <= cc.K_FAR_USE and sum(trips) > cc.K_FAR_USE  # through the list, which fills up
        assert slab.ball_chunks(q, keys, counts) > cc.K_FAR_USE
    # the brim blocks: one trip of exactly kFarUse / kFarUse + 1 chunks
    for q, (_, _, _, chunks) in zip(slab.brim_queries, cc.BRIM_BLOCKS):
        assert slab.points_in_27(q) == 0
        assert slab.row_trip_totals(q) == [chunks] and slab.ball_chunks(q, keys, counts) == chunks
    # the unseeded class: more candidates around the query than the search pass's table takes, in round 1 already
    for q in slab.in_slab:
        assert slab.points_in_27(q) > cc.SEARCH_TABLE_POINTS
        assert slab.chunks_in_nearest_8(q) > cc.SEARCH_TABLE_CHUNKS


def test_tie_share_and_classes(slab):
    r = cc.Reference(slab.tree, slab.queries)
    tie = slab.group == "tie"
    for copies in (2, 4):
        assert r.tie56[tie][slab.tie_kind == copies].mean() >= 0.5
    # four copies: the 5th distance is the 7th as well - what the search pass flags as ambiguous
    _, d8, c8 = slab.tree.knn(slab.queries[tie][slab.tie_kind == 4], k=7, threads=4)
    assert ((c8 == 7) & (d8[:, 4] == d8[:, 6])).mean() >= 0.5
    assert r.tie56[~tie].sum() == 0
    assert cc.classify_U(r)[np.isin(slab.group, ("U", "facing_a", "facing_b"))].all()
    assert cc.classify_F(r)[slab.group == "F"].all() and (slab.group == "F").sum() == cc.F_N
    # the brim queries' five neighbours are the five points of the last cell listed
    brim = slab.group == "brim"
    assert (r.cnt[brim] == 5).all() and (r.d5[brim] < 0.36).all()
    # every mix of the slab scans stays inside the flagged range of the path it is meant for
    for mix, (lo_path, hi_path) in cc.SLAB_MIX_RANGE.items():
        scan, ids, sure, at_most = slab.scan(mix)
        assert lo_path <= sure <= at_most <= hi_path and len(scan) == len(ids) <= 9000
        assert np.array_equal(scan[:, :3], slab.queries[ids]) and (slab.group[ids] == "F").sum() == cc.F_N


def _same(ref, bp, bd, bc, sel):
    cnt = ref.cnt[sel]
    assert np.array_equal(np.minimum(bc, 5), cnt)
    valid = np.arange(5)[None, :] < cnt[:, None]
    assert np.array_equal(bd[:, :5].view(np.uint32)[valid], ref.d2[sel].view(np.uint32)[valid])
    strict = ~ref.tie56[sel]
    assert np.array_equal(bp[:, :5][strict].view(np.uint32)[valid[strict]], ref.pts[sel][strict].view(np.uint32)[valid[strict]])


def test_brute_force_is_the_trees(hole, slab, oracle):
    sel = np.r_[np.arange(0, cc.F_N, 30), cc.F_N + np.arange(cc.BRUTE_SAMPLE)]
    for variant in ("win", "hashed"):
        tree = oracle.Tree("oracle")
        tree.build(hole.maps[variant])
        ref = cc.Reference(tree, hole.queries)
        bp, bd, bc = cc.brute_knn(hole.queries, hole.maps[variant], sel)
        _same(ref, bp, bd, bc, sel)
        assert ((bc >= 6) & (bd[:, 4] == bd[:, 5])).sum() == 0
    sel = np.flatnonzero(slab.group != "F")
    ref = cc.Reference(slab.tree, slab.queries)
    bp, bd, bc = cc.brute_knn(slab.queries, slab.map, sel)
    _same(ref, bp, bd, bc, sel)
    assert np.array_equal((bc >= 6) & (bd[:, 4] == bd[:, 5]), ref.tie56[sel])
    if oracle.ref_available():
        for mp, q, sel in ((hole.maps["win"], hole.queries, np.r_[np.arange(0, cc.F_N, 30), cc.F_N + np.arange(cc.BRUTE_SAMPLE)]), (slab.map, slab.queries, sel)):
            rt = oracle.Tree("ref")
            rt.build(mp)
            ref = cc.Reference(rt, q)
            bp, bd, bc = cc.brute_knn(q, mp, sel)
            _same(ref, bp, bd, bc, sel)
