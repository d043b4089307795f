"""lii_map_delete_points / _dev, lii_map_range and lii_map_box_search on the device against the reference tree and numpy.  Every
comparison is of float BITS (multisets of rows, MC.same_multiset); nothing here carries a tolerance.

The models.  A duplicate-free map: the UNMODIFIED reference tree follows a point delete through Delete_Point_Boxes with the one-ulp box
[p, nextafter(p, +inf)) per listed point (held to the tree on the CPU in test_map_points_abi.py); listed coordinates are never zero.  A map
with bit-equal twins: the numpy multiset difference (rows with multiplicity)."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

import map_removed_cases as MC

pytestmark = pytest.mark.gpu

INVALID, STATE, CAPACITY = -1, -5, -4


def _registrar(**kw):
    import lidar_imu_init_amd as lii
    return lii.Registrar(**{**dict(max_scan_points=20_000, max_map_points=60_000, filter_size_map=0.2), **kw})


def _unique_points(rng, n, lo=-10.0, hi=10.0):
    p = np.unique(rng.uniform(lo, hi, (n, 3)).astype(np.float32), axis=0)
    p = p[(p != 0).all(axis=1)]
    return np.ascontiguousarray(p[rng.permutation(len(p))])


def _ms_minus(a, b):
    """(a minus b as multisets of rows, number of rows removed): every row of b takes one bit-equal row of a, if one is left."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
    need = collections.Counter(r.tobytes() for r in np.ascontiguousarray(b, np.float32).reshape(-1, 3))
    keep = np.ones(len(a), bool)
    for i, r in enumerate(a):
        k = r.tobytes()
        if need.get(k, 0) > 0:
            need[k] -= 1
            keep[i] = False
    return a[keep], int((~keep).sum())


def _one_ulp_boxes(p):
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    assert (p != 0).all()
    return np.concatenate([p, np.nextafter(p, np.float32(np.inf))], axis=1).astype(np.float32)


def _range_of(p):
    return np.concatenate([p.min(axis=0), p.max(axis=0)]).astype(np.float32)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _code(fn, *a, **kw):
    import lidar_imu_init_amd as lii
    try:
        fn(*a, **kw)
        return 0
    except lii.LIIError as e:
        return e.code


def _search(reg, oracle, q):
    """One searching pass for the points q; returns (neighbour points, counts)."""
    import lidar_imu_init_amd as lii
    reg.scan_upload(np.c_[q, np.zeros(len(q), np.float32)])
    n = reg.downsample_skip()
    reg.iekf_iterate(lii.State(oracle.state_init()), True, False)
    nb, cnt, _ = reg.neighbors(n)
    return nb, cnt


def _assert_lists_of(oracle, nb, cnt, q, survivors):
    t = oracle.Tree("oracle")
    t.build(survivors)
    pts, _, rc = t.knn(q, threads=4)
    t.close()
    assert np.array_equal(cnt, rc)
    for k in range(5):
        m = cnt > k
        assert np.array_equal(nb[m, k], pts[m, k])


# ------------------------------------------------------------------------------------------------ 1
def test_listed_points_against_the_reference_tree(oracle):
    rng = np.random.default_rng(31)
    base = _unique_points(rng, 20_000)
    pick = rng.choice(len(base), 257, replace=False)
    moved = base[rng.choice(len(base), 20, replace=False)] + np.float32(1e-3)
    absent = np.concatenate([rng.uniform(-10, 10, (20, 3)).astype(np.float32), moved])
    lst = np.concatenate([base[pick], absent, np.array([[np.nan, 1.0, 2.0]], np.float32)]).astype(np.float32)
    lst = lst[rng.permutation(len(lst))]
    want, n_want = _ms_minus(base, lst)
    assert n_want == 257
    reg = _registrar()
    reg.map_build(base)
    n = reg.map_delete_points(lst)
    print(f"listed {len(lst)} points (257 stored): deleted {n}, map {reg.map_size()} of {len(base)}")
    assert n == 257 and reg.map_size() == len(base) - 257
    got = reg.map_download()
    assert MC.same_multiset(got, want)
    q = rng.uniform(-10, 10, (4000, 3)).astype(np.float32)
    _, d2, cnt = reg.map_nearest(q, k=5)
    if oracle.ref_available():
        tree = oracle.Tree("ref")
        tree.build(base)
        assert tree.delete_boxes(_one_ulp_boxes(base[pick])) == 257
        assert tree.validnum() == reg.map_size()
        assert MC.same_multiset(tree.flatten(), got)
        tree.close()
    t2 = oracle.Tree("ref" if oracle.ref_available() else "oracle")
    t2.build(want)
    _, rd2, rc = t2.knn(q, k=5)
    t2.close()
    assert np.array_equal(cnt, rc) and _same_bits(d2, rd2)
    assert reg.map_delete_points(lst) == 0 and reg.map_size() == len(base) - 257  # the same list again: nothing is left of it
    assert MC.same_multiset(reg.map_download(), want)
    reg.close()


# ------------------------------------------------------------------------------------------------ 2
def _list_of(rng, stored, n):
    """n listed points: four in five stored (distinct), the rest absent; shuffled."""
    k = min(len(stored), (4 * n + 4) // 5)
    lst = np.concatenate([stored[rng.choice(len(stored), k, replace=False)], rng.uniform(-10, 10, (n - k, 3)).astype(np.float32)])
    return np.ascontiguousarray(lst[rng.permutation(n)], np.float32), k


def test_list_sizes():
    rng = np.random.default_rng(32)
    base = _unique_points(rng, 12_000)
    reg = _registrar()
    for n in (0, 1, 63, 64, 65, 256, 257, 4097):
        reg.map_build(base)
        lst, k = _list_of(rng, base, n)
        want, n_want = _ms_minus(base, lst)
        got_n = reg.map_delete_points(lst)
        print(f"list of {n}: {k} stored, deleted {got_n}")
        assert n_want == k and got_n == k and reg.map_size() == len(base) - k
        assert MC.same_multiset(reg.map_download(), want)
    reg.close()


def test_list_longer_than_a_chunk():
    rng = np.random.default_rng(33)
    base = _unique_points(rng, 70_000, -20.0, 20.0)
    assert 69_000 < len(base) <= 70_000
    reg = _registrar(max_map_points=80_000)
    reg.map_build(base)
    lst, k = _list_of(rng, base, 65_537)
    lst[-1] = lst[0] = base[7]  # one stored point at both ends of the list, in different chunks: it goes once
    want, n_want = _ms_minus(base, lst)
    got_n = reg.map_delete_points(lst)
    print(f"list of {len(lst)} out of {len(base)}: deleted {got_n} (numpy {n_want})")
    assert got_n == n_want and reg.map_size() == len(base) - n_want
    assert MC.same_multiset(reg.map_download(), want)
    reg.close()


# ------------------------------------------------------------------------------------------------ 3
def test_twins():
    rng = np.random.default_rng(34)
    base = _unique_points(rng, 2_000, -5.0, 5.0)[:2000]
    reg = _registrar()
    reg.map_build(base)
    n0 = reg.map_size()
    reg.map_add_points(base[:500], False)
    reg.map_add_points(base[:100], False)
    assert reg.map_size() == n0 + 600  # the precondition: the map holds twins
    model = np.concatenate([base, base[:500], base[:100]])
    assert MC.same_multiset(reg.map_download(), model)
    filler = rng.uniform(20, 30, (400, 3)).astype(np.float32)  # absent

    def step(lst, expect, stays):
        nonlocal model
        lst = np.ascontiguousarray(lst, np.float32)
        model, n_model = _ms_minus(model, lst)
        n = reg.map_delete_points(lst)
        assert n == n_model == expect, (n, n_model, expect)
        got = reg.map_download()
        assert MC.same_multiset(got, model)
        for p, c in stays:
            assert int((got.view(np.uint32) == p.view(np.uint32)).all(axis=1).sum()) == c

    twice, thrice = base[100:500], base[:100]
    step(twice[:1], 1, [(twice[0], 1)])  # one copy of a twice-stored point: one stays
    step(np.concatenate([twice[1:2], twice[1:2]]), 2, [(twice[1], 0)])  # two copies, adjacent
    step(np.concatenate([twice[2:3], filler, twice[2:3]]), 2, [(twice[2], 0)])  # two copies more than 256 entries apart: another workgroup
    step(np.repeat(twice[3:4], 4, axis=0), 2, [(twice[3], 0)])  # four copies of a twice-stored point: two go
    step(np.repeat(thrice[:1], 3, axis=0), 3, [(thrice[0], 0)])  # three copies of a thrice-stored point
    step(np.concatenate([np.repeat(thrice[1:2], 2, axis=0), filler[:300], twice[4:5]]), 3, [(thrice[1], 1), (twice[4], 1)])
    reg.close()


# ------------------------------------------------------------------------------------------------ 4
def test_same_point_rule_across_cell_and_block_seams():
    cs = np.float32(0.5)
    rng = np.random.default_rng(35)
    below = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))
    stored = np.array([[1.5, 0.2, 0.3],      # a cell face on x
                       [1.5, 1.5, 1.5],      # ... on all three axes: the listed point's interval spans eight cells
                       [4.0, 12.3, 12.3],    # a block face on x; the block below it holds nothing
                       [4.0, 4.0, -4.0],     # a block corner: eight blocks, seven of them not in the table
                       [0.25, 0.25, 0.25]], np.float32)
    far = rng.uniform(-10, -5, (50, 3)).astype(np.float32)
    pts = np.concatenate([stored, far])
    listed = np.array([[below(1.5), 0.2, 0.3], [below(1.5), below(1.5), below(1.5)], [below(4.0), 12.3, 12.3],
                       [below(4.0), below(4.0), below(-4.0)]], np.float32)
    # the preconditions: another cell / another block, and inside same_point's 1e-6
    cell = lambda p: np.floor(p / cs).astype(np.int64)
    assert (cell(listed[0]) != cell(stored[0])).sum() == 1 and (cell(listed[1]) != cell(stored[1])).all()
    assert (cell(listed[2]) >> 3 != cell(stored[2]) >> 3).sum() == 1 and (cell(listed[3]) >> 3 != cell(stored[3]) >> 3).all()
    assert (np.abs(listed - stored[:4]).astype(np.float64) < 1e-6).all() and (listed != stored[:4]).any(axis=1).all()
    blk = cell(pts) >> 3
    assert not (blk == cell(listed[2]) >> 3).all(axis=1).any()  # the block below x = 4.0 is not in the table
    reg = _registrar(map_cell_size=float(cs))
    reg.map_build(pts)
    for i in range(4):
        assert reg.map_delete_points(listed[i:i + 1]) == 1, i
        assert MC.same_multiset(reg.map_download(), np.delete(pts, np.arange(i + 1), axis=0))
    off = stored[4:5].copy()
    off[0, 0] += np.float32(2e-6)
    assert np.float64(abs(off[0, 0] - stored[4, 0])) >= 1e-6
    assert reg.map_delete_points(off) == 0 and reg.map_size() == len(pts) - 4
    assert reg.map_delete_points(stored[4:5]) == 1
    reg.close()


# ------------------------------------------------------------------------------------------------ 5
def test_mixed_sequence_against_the_reference_tree(oracle):
    rng = np.random.default_rng(36)
    have_ref = oracle.ref_available()
    reg = _registrar()
    first = _unique_points(rng, 600, -3.0, 3.0)
    reg.map_build(first)
    tree = None
    if have_ref:
        tree = oracle.Tree("ref", downsample=0.2)
        tree.build(first)
    for rnd in range(30):
        c = np.array([0.4 * rnd, 0.2 * rnd, 0.0])
        batch = (rng.uniform(-3, 3, (300, 3)) + c).astype(np.float32)
        reg.map_add_points(batch, True)
        cur = reg.map_download()
        if tree is not None:
            tree.add_points(batch, True)
            assert tree.validnum() == len(cur), rnd
        sel = cur[rng.choice(len(cur), max(len(cur) // 20, 1), replace=False)]
        model, n_model = _ms_minus(cur, sel)
        assert n_model == len(sel)  # (down-sampled adds leave no twins)
        assert reg.map_delete_points(sel) == len(sel)
        lo = (rng.uniform(-3, 2, 3) + c).astype(np.float32)
        box = np.concatenate([lo, lo + np.float32(1.0)]).astype(np.float32)[None]
        dead = MC.in_boxes(model, box)
        assert reg.map_delete_boxes(box) == int(dead.sum())
        model = model[~dead]
        got = reg.map_download()
        assert MC.same_multiset(got, model), rnd
        assert reg.map_size() == len(model)
        assert _same_bits(reg.map_range(), _range_of(model)), rnd
        if tree is not None:
            assert tree.delete_boxes(_one_ulp_boxes(sel)) == len(sel)
            assert tree.delete_boxes(box) == int(dead.sum())
            assert tree.validnum() == len(model)
            assert MC.same_multiset(tree.flatten(settle_ms=30), got), rnd
    if tree is not None:
        tree.close()
    print(f"30 rounds: the map holds {len(model)} points")
    q = (rng.uniform(-3, 3, (3000, 3)) + np.array([6.0, 3.0, 0.0])).astype(np.float32)
    nb, cnt = _search(reg, oracle, q)
    _assert_lists_of(oracle, nb, cnt, q, model)
    reg.close()


# ------------------------------------------------------------------------------------------------ 6
def test_history_collects_what_a_point_delete_removes():
    rng = np.random.default_rng(37)
    base = _unique_points(rng, 6_000)
    reg = _registrar()
    reg.map_build(base)
    reg.map_removed_set(4096)
    a = base[rng.choice(2000, 300, replace=False)]
    lst = np.concatenate([a, rng.uniform(-10, 10, (30, 3)).astype(np.float32)])
    assert reg.map_delete_points(lst) == 300
    assert reg.map_removed_get() == {"capacity": 4096, "held": 300, "collected_total": 300, "lost_total": 0}
    assert MC.same_multiset(reg.map_removed_acquire(clear=True), a)
    # a buffer too small: the delete completes, what finds no room is counted
    reg.map_removed_set(100)
    b = base[2000 + rng.choice(2000, 300, replace=False)]
    assert reg.map_delete_points(b) == 300
    assert reg.map_removed_get() == {"capacity": 100, "held": 100, "collected_total": 100, "lost_total": 200}
    want, _ = _ms_minus(_ms_minus(base, a)[0], b)
    assert MC.same_multiset(reg.map_download(), want)
    assert _code(reg.map_removed_acquire) == CAPACITY and _code(reg.map_removed_acquire, clear=True) == CAPACITY
    assert reg.map_removed_get()["held"] == 100
    got = reg.map_removed_acquire(clear=True, strict=False)
    assert len(got) == 100 and _ms_minus(b, got)[1] == 100  # a sub-multiset of what went
    assert len(reg.map_removed_acquire()) == 0
    assert reg.map_removed_get() == {"capacity": 100, "held": 0, "collected_total": 100, "lost_total": 200}
    # the order off: nothing is collected
    reg.map_removed_set(0)
    assert reg.map_delete_points(base[4000:4050]) == 50
    assert reg.map_removed_get() == {"capacity": 0, "held": 0, "collected_total": 100, "lost_total": 200}
    reg.close()


# ------------------------------------------------------------------------------------------------ 7
def test_dev_form(oracle):
    rng = np.random.default_rng(38)
    base = _unique_points(rng, 20_000)
    reg = _registrar()
    reg.map_build(base)
    q = rng.uniform(-3, 3, (2000, 3)).astype(np.float32)
    nb0, cnt0 = _search(reg, oracle, q)
    near = np.unique(nb0[cnt0 > 0, 0], axis=0)  # stored points the lists of that search hold
    lst = np.concatenate([near[:400], base[rng.choice(len(base), 300, replace=False)], rng.uniform(-10, 10, (50, 3)).astype(np.float32)])
    want, n_want = _ms_minus(base, lst)
    rec = np.zeros((len(lst), 4), np.float32)  # stride 16
    rec[:, :3] = lst
    rec[:, 3] = 7.0
    d = reg.dev_alloc(rec.nbytes)
    reg.dev_upload(d, rec)
    import lidar_imu_init_amd as lii
    st = lii.State(oracle.state_init())
    reg.iekf_iterate(st, False, False)  # the lists of the search are still served
    reg.map_delete_points_dev(d, len(lst), stride_bytes=16)
    # nobody knows yet whether anything went: the lists of the earlier search are not used again
    assert _code(reg.iekf_iterate, st, False, False) == STATE
    reg.synchronize()
    assert reg.map_size() == len(base) - n_want
    assert MC.same_multiset(reg.map_download(), want)
    nb1, cnt1 = _search(reg, oracle, q)  # a registration behind it searches anew: neighbours come from the survivors only
    _assert_lists_of(oracle, nb1, cnt1, q, want)
    assert not np.array_equal(nb0, nb1)
    # enqueue, then a search with nothing in between: the search joins the delete
    lst2 = np.unique(nb1[cnt1 > 0, 0], axis=0)[:200]
    d2 = reg.dev_alloc(lst2.nbytes)
    reg.dev_upload(d2, lst2)
    reg.map_delete_points_dev(d2, len(lst2))
    nb2, cnt2 = _search(reg, oracle, q)
    want2, n2 = _ms_minus(want, lst2)
    assert n2 == len(lst2)
    _assert_lists_of(oracle, nb2, cnt2, q, want2)
    assert reg.map_size() == len(want2)
    reg.close()


# ------------------------------------------------------------------------------------------------ 8
def test_map_range():
    rng = np.random.default_rng(39)
    base = _unique_points(rng, 9_000)
    reg = _registrar()
    zeros = np.zeros(6, np.float32)
    assert _same_bits(reg.map_range(), zeros)  # no map
    reg.map_build(base)
    assert _same_bits(reg.map_range(), _range_of(base))
    extreme = np.unique(np.concatenate([base.argmin(axis=0), base.argmax(axis=0)]))
    assert len(extreme) == 6
    assert reg.map_delete_points(base[extreme]) == 6
    rest = np.delete(base, extreme, axis=0)
    r = reg.map_range()
    assert _same_bits(r, _range_of(rest)) and not (r == _range_of(base)).any()
    reg.map_reset()
    assert _same_bits(reg.map_range(), zeros)
    reg.close()


# ------------------------------------------------------------------------------------------------ 9
def test_map_box_search(oracle):
    rng = np.random.default_rng(12)
    base = rng.uniform(-10, 10, (30_000, 3)).astype(np.float32)
    # the boxes and face points of test_delete_boxes_matches_the_reference_tree, an overlapping pair and a box outside the map
    boxes = np.array([[-2, -2, -2, 2, 2, 2], [5, -10, -10, 10, 10, 0.5], [-9.5, 3, 3, -9.0, 3.5, 3.5], [20, 20, 20, 30, 30, 30],
                      [1, 1, 1, 5, 5, 5], [3, 3, 3, 7, 7, 7]], np.float32)
    base[:6] = [[-2, 0, 0], [2, 0, 0], [0, -2, 1.999], [0, 2, 0], [5, 0, 0.5], [5, 0, 0.4999]]
    inside = MC.in_boxes(base, boxes)
    assert inside[[0, 2, 5]].all() and not inside[[1, 3, 4]].any()  # the lower face is in, the upper one is out
    hits = sum(MC.in_boxes(base, boxes[i:i + 1]).astype(int) for i in range(len(boxes)))
    assert (hits >= 2).sum() > 10 and not MC.in_boxes(base, boxes[3:4]).any()
    reg = _registrar()
    reg.map_build(base)
    q = rng.uniform(-3, 3, (2000, 3)).astype(np.float32)
    nb0, cnt0 = _search(reg, oracle, q)
    got = reg.map_box_search(boxes)
    print(f"{len(boxes)} boxes hold {len(got)} of {len(base)} points (numpy {int(inside.sum())})")
    assert MC.same_multiset(got, base[inside])
    assert len(reg.map_box_search(np.zeros((0, 6), np.float32))) == 0 and len(reg.map_box_search(boxes[3:4])) == 0
    one = reg.map_box_search(boxes[4:5])
    assert MC.same_multiset(one, base[MC.in_boxes(base, boxes[4:5])])
    # capacity: the rule of lii_map_download - *n is the full count; NULL: the count only; too small: LII_ERR_CAPACITY, nothing written
    L, h = reg.L, reg.h
    b = np.ascontiguousarray(boxes)
    n = C.c_int32(-1)
    assert L.lii_map_box_search(h, b.ctypes.data, len(b), None, 0, C.byref(n)) == 0 and n.value == int(inside.sum())
    small = np.full((n.value - 1, 3), 7.0, np.float32)
    n = C.c_int32(-1)
    assert L.lii_map_box_search(h, b.ctypes.data, len(b), small.ctypes.data, len(small), C.byref(n)) == CAPACITY
    assert n.value == int(inside.sum()) and (small == 7.0).all()
    n = C.c_int32(-1)
    assert L.lii_map_box_search(h, None, 0, small.ctypes.data, len(small), C.byref(n)) == 0 and n.value == 0
    # the search changed nothing: the size, and the lists of the earlier search are still served
    import lidar_imu_init_amd as lii
    assert reg.map_size() == len(base)
    reg.iekf_iterate(lii.State(oracle.state_init()), False, False)
    nb1, cnt1, _ = reg.neighbors(len(q))
    assert np.array_equal(nb0, nb1) and np.array_equal(cnt0, cnt1)
    # ... and what it returned is what the delete of the same boxes removes
    reg.map_removed_set(len(base))
    assert reg.map_delete_boxes(boxes) == len(got)
    assert MC.same_multiset(reg.map_removed_acquire(), got)
    assert len(reg.map_box_search(boxes)) == 0
    reg.close()


# ------------------------------------------------------------------------------------------------ 10
def test_refusals():
    rng = np.random.default_rng(40)
    base = _unique_points(rng, 3_000)
    reg = _registrar()
    reg.map_build(base)
    L, h = reg.L, reg.h
    n = C.c_int32(-1)
    p = np.ascontiguousarray(base[:10])
    d = reg.dev_alloc(p.nbytes)
    reg.dev_upload(d, p)
    for stride in (0, 8, 14, -12):
        assert L.lii_map_delete_points(h, p.ctypes.data, len(p), stride, C.byref(n)) == INVALID
        assert L.lii_map_delete_points_dev(h, d, len(p), stride) == INVALID
    assert L.lii_map_delete_points(h, None, 3, 12, C.byref(n)) == INVALID
    assert L.lii_map_delete_points_dev(h, None, 3, 12) == INVALID
    assert L.lii_map_delete_points(h, p.ctypes.data, -1, 12, C.byref(n)) == INVALID
    boxes = np.tile(np.array([-20, -20, -20, 20, 20, 20], np.float32), (4097, 1))
    out = np.zeros((len(base), 3), np.float32)
    assert L.lii_map_box_search(h, boxes.ctypes.data, 4097, out.ctypes.data, len(out), C.byref(n)) == INVALID
    assert L.lii_map_box_search(h, None, 2, out.ctypes.data, len(out), C.byref(n)) == INVALID
    assert L.lii_map_box_search(h, boxes.ctypes.data, 1, out.ctypes.data, len(out), None) == INVALID
    assert L.lii_map_range(h, None) == INVALID
    assert reg.map_size() == len(base) and MC.same_multiset(reg.map_download(), base)  # nothing changed
    # what is no error: NULL with n == 0, an empty list, a point that is not there, 4096 boxes
    assert L.lii_map_delete_points(h, None, 0, 12, None) == 0
    assert reg.map_delete_points(np.zeros((0, 3), np.float32)) == 0
    assert reg.map_delete_points(np.array([[50.0, 50.0, 50.0], [np.inf, 1.0, 1.0], [1e30, -1e30, 1.0]], np.float32)) == 0
    assert L.lii_map_box_search(h, boxes.ctypes.data, 4096, None, 0, C.byref(n)) == 0 and n.value == len(base)
    assert L.lii_map_delete_points(h, p.ctypes.data, 4, 12, None) == 0 and reg.map_size() == len(base) - 4  # n_deleted may be NULL
    reg.map_reset()
    assert reg.map_delete_points(p) == 0 and len(reg.map_box_search(boxes[:1])) == 0  # an empty map
    reg.map_delete_points_dev(d, len(p))
    assert reg.map_size() == 0
    reg.close()
    # ... and the largest requests the argument checks let through, next to each other in one handle
    _largest_requests_side_by_side()


def _canon(a):
    """The rows of a (n, 3) float32 array in the order of their bits, as bytes: equal for equal multisets of rows."""
    v = np.ascontiguousarray(a, np.float32).reshape(-1, 3).view(np.uint32)
    return v[np.lexsort(v.T[::-1])].tobytes()


def _largest_requests_side_by_side():
    """4096 boxes into lii_map_delete_boxes and lii_map_box_search (lii_map_size and lii_map_range between them) and 63 IMU samples into
    lii_imu_propagate, on ONE handle, the delete in front of the others and behind them: every call gives the bits it gives alone on a
    fresh handle, and those are numpy's (min <= p < max; the recorded reference run of the n63 case is held in test_gpu_imu_propagate.py)."""
    import lidar_imu_init_amd as lii
    rng = np.random.default_rng(42)
    base = _unique_points(rng, 2_000)
    outside = lambda n: _one_ulp_boxes(rng.uniform(20, 30, (n, 3)).astype(np.float32))
    del_boxes = np.concatenate([_one_ulp_boxes(base[rng.choice(len(base), 300, replace=False)]), outside(4096 - 300)])
    del_boxes = np.ascontiguousarray(del_boxes[rng.permutation(4096)])
    lo = rng.uniform(-10, 8, (96, 3)).astype(np.float32)
    find_boxes = np.concatenate([_one_ulp_boxes(base[rng.choice(len(base), 500, replace=False)]), np.c_[lo, lo + np.float32(2.0)], outside(3500)])
    find_boxes = np.ascontiguousarray(find_boxes[rng.permutation(4096)], np.float32)
    assert del_boxes.shape == find_boxes.shape == (4096, 6)
    dead = MC.in_boxes(base, del_boxes)
    left = base[~dead]
    assert int(dead.sum()) == 300
    F = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imu", "reference_propagation.npz"))
    c = {k: F[f"lio/n63/in/{k}"] for k in ("state", "imu", "last_imu", "last_end", "acc_s_last", "angvel_last", "beg", "pts", "cov_gyr", "cov_acc")}
    assert len(c["imu"]) == 63

    def fresh(map_pts=None):
        reg = _registrar(max_scan_points=1_000, max_map_points=16_000)
        if map_pts is not None:
            reg.map_build(map_pts)
        return reg

    def delete(reg):
        return reg.map_delete_boxes(del_boxes), _canon(reg.map_download())

    def imu(reg):
        reg.set_imu_noise(cov_gyr=c["cov_gyr"], cov_acc=c["cov_acc"], mean_acc_norm=9.805)
        reg.imu_carry = dict(last_imu=c["last_imu"], acc_s_last=c["acc_s_last"], angvel_last=c["angvel_last"], last_lidar_end_time=float(c["last_end"]))
        beg = float(c["beg"])
        st, poses = reg.propagate_imu(c["imu"], beg, beg + float(c["pts"][-1, 3]) / 1000.0, lii.State(c["state"]))
        carry = reg.imu_carry
        assert len(poses) == 64
        return st.pod.tobytes(), poses.tobytes(), np.r_[carry["last_imu"], carry["acc_s_last"], carry["angvel_last"], carry["last_lidar_end_time"]].tobytes()

    queries = (("size", lambda reg: reg.map_size()), ("range", lambda reg: reg.map_range().tobytes()),
               ("search", lambda reg: _canon(reg.map_box_search(find_boxes))))

    def alone(call, map_pts=None):
        reg = fresh(map_pts)
        out = call(reg)
        reg.close()
        return out

    solo = {"delete": alone(delete, base), "imu": alone(imu)}
    assert solo["delete"] == (300, _canon(left))
    for tag, m in (("whole", base), ("left", left)):
        for name, call in queries:
            solo[tag, name] = alone(call, m)
        assert solo[tag, "size"] == len(m) and solo[tag, "range"] == _range_of(m).tobytes()
        assert solo[tag, "search"] == _canon(m[MC.in_boxes(m, find_boxes)])
    print(f"4096 boxes delete {solo['delete'][0]} of {len(base)} points; 4096 boxes hold {len(solo['whole', 'search']) // 12} / {len(solo['left', 'search']) // 12} points")
    assert 500 < len(solo["whole", "search"]) // 12 > len(solo["left", "search"]) // 12
    for delete_first in (True, False):
        reg = fresh(base)
        if delete_first:
            assert delete(reg) == solo["delete"]
        tag = "left" if delete_first else "whole"
        for name, call in queries:
            assert call(reg) == solo[tag, name], (delete_first, name)
        assert imu(reg) == solo["imu"], delete_first
        if not delete_first:
            assert delete(reg) == solo["delete"]
        reg.close()


def test_under_host_solve():
    rng = np.random.default_rng(41)
    base = _unique_points(rng, 3_000)
    lst = base[rng.choice(len(base), 100, replace=False)]
    want, _ = _ms_minus(base, lst)
    old = os.environ.get("LII_TEST")
    os.environ["LII_TEST"] = "host_solve"
    try:
        reg = _registrar()
    finally:
        os.environ.pop("LII_TEST", None)
        if old is not None:
            os.environ["LII_TEST"] = old
    reg.map_build(base)
    assert reg.map_delete_points(lst) == 100 and MC.same_multiset(reg.map_download(), want)
    assert MC.same_multiset(reg.map_box_search(np.array([[-20, -20, -20, 20, 20, 20]], np.float32)), want)
    reg.close()
