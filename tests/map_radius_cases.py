"""What the ball-query tests share (test_map_radius_ref.py on the CPU, test_gpu_map_radius.py on the device): the per-query brute-force
ball and the comparison of an (offsets, pts, d2) answer with it.

The brute force is map_nearest_cases.d2_f32 - the reference's calc_dist written out in float32 - over all map points; per query it keeps
EVERY point with d2 <= the bound the query is computed for, ascending in (d2, index), once per (map, query set).  A case cuts every
segment at its max_dist (the float d2 against the double max_dist, inclusive, as Search compares).  All comparisons are exact: offsets
equal, per query the multiset of d2 bits equal, per query the multiset of point rows (bits) equal."""
import numpy as np

from map_nearest_cases import d2_f32, query_set

MAX_DISTS_TREE = (1.0, 5.0, 30.0)  # what the reference tree serves as a ball (>= 1)
FAR_EVERY_GPU, FAR_EVERY_REF = 4, 10  # max_dist 30: every 4th query on the device, every 10th against the tree on the CPU


class Balls:
    """CSR over the queries: idx / d2 of every map point with d2 <= d2_max[i], rows off[i] .. off[i + 1] - 1, ascending in (d2, index).
    d2_max: one bound, or one per query (a query with bound < 0 is not computed: its segment is empty and it must not be asked for)."""

    def __init__(self, q, pts, d2_max, chunk=64):
        self.q = np.asarray(q, np.float32)
        self.pts = np.ascontiguousarray(pts, np.float32)
        n = len(self.q)
        self.bound = np.broadcast_to(np.asarray(d2_max, np.float64), (n,)).copy()
        idx, d2, cnt = [], [], np.zeros(n, np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            for a in range(0, n, chunk):
                d = d2_f32(self.q[a:a + chunk], self.pts)
                ok = d.astype(np.float64) <= self.bound[a:a + chunk, None]  # (a NaN query: nothing qualifies)
                r, c = np.nonzero(ok)
                dv = d[r, c]
                order = np.lexsort((c, dv, r))
                idx.append(c[order].astype(np.int32))
                d2.append(dv[order])
                cnt[a:a + chunk] = np.bincount(r, minlength=len(d))
        self.off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        self.idx = np.concatenate(idx) if idx else np.zeros(0, np.int32)
        self.d2 = np.concatenate(d2) if d2 else np.zeros(0, np.float32)

    def case(self, max_dist, sel=None):
        """(offsets (m + 1,), idx, d2) of the queries `sel` (all by default) at max_dist <= their bound."""
        sel = np.arange(len(self.q)) if sel is None else np.asarray(sel)
        assert np.all(self.bound[sel] >= float(max_dist)), "the brute force was not computed that far for these queries"
        seg = np.repeat(np.arange(len(self.q)), np.diff(self.off))
        pick = np.zeros(len(self.q), bool)
        pick[sel] = True
        keep = pick[seg] & (self.d2.astype(np.float64) <= float(max_dist))
        cnt = np.bincount(seg[keep], minlength=len(self.q))[sel]
        if len(sel) and np.any(np.diff(sel) < 0):
            raise ValueError("sel must ascend")
        return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), self.idx[keep], self.d2[keep]


_cache = {}


def small_world_balls(small_world):
    """The 2 000-query set over the suite's hall map and its balls, once per session: up to d2 = 30 for every 4th and every 10th
    query, up to 5 for the others."""
    if "sw" not in _cache:
        hall, map_pts = small_world
        map_pts = np.ascontiguousarray(map_pts, np.float32)
        q = query_set(hall, map_pts)
        i = np.arange(len(q))
        bound = np.where((i % FAR_EVERY_GPU == 0) | (i % FAR_EVERY_REF == 0), 30.0, 5.0)
        _cache["sw"] = (q, Balls(q, map_pts, bound))
    return _cache["sw"]


def _sorted_rows(off, cols):
    """rows of every segment sorted by `cols` (most significant first)"""
    seg = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return np.lexsort(tuple(reversed(cols)) + (seg,)) if len(seg) else np.zeros(0, np.int64)


def check_radius(offsets, pts, d2, expected, map_pts, who, q=None):
    """Holds (offsets, pts, d2) to expected = (offsets, idx into map_pts, d2): offsets equal (so counts and total), per query the
    multiset of d2 bits equal, per query the multiset of point rows equal; with the queries `q`, every row pairs a point with ITS d2.
    pts / d2 may be None (not asked for).  Prints the figures before it asserts."""
    eo, ei, ed = expected
    offsets = np.asarray(offsets)
    n_off = int(np.count_nonzero(offsets != eo)) if offsets.shape == eo.shape else -1
    print(f"{who}: {len(eo) - 1} queries, {int(eo[-1])} rows expected, {int(offsets[-1]) if len(offsets) else -1} returned, offsets differ {n_off}, "
          f"largest ball {int(np.diff(eo).max()) if len(eo) > 1 else 0}, empty balls {int((np.diff(eo) == 0).sum())}")
    assert offsets.dtype == np.int64 and offsets.shape == eo.shape and n_off == 0, f"{who}: offsets differ from the expected ones"
    assert offsets[0] == 0 and np.all(np.diff(offsets) >= 0)
    if d2 is not None:
        assert d2.shape == (eo[-1],) and d2.dtype == np.float32
        gb, eb = d2.view(np.uint32), np.asarray(ed, np.float32).view(np.uint32)
        same = np.array_equal(gb[_sorted_rows(eo, (gb,))], eb[_sorted_rows(eo, (eb,))])
        assert same, f"{who}: the d2 bits of some query differ from the expected multiset"
    if pts is not None:
        assert pts.shape == (eo[-1], 3) and pts.dtype == np.float32
        g = np.ascontiguousarray(pts).view(np.uint32)
        e = np.ascontiguousarray(np.asarray(map_pts, np.float32)[ei]).view(np.uint32).reshape(-1, 3)
        gs = g[_sorted_rows(eo, (g[:, 0], g[:, 1], g[:, 2]))]
        es = e[_sorted_rows(eo, (e[:, 0], e[:, 1], e[:, 2]))]
        assert np.array_equal(gs, es), f"{who}: the point rows of some query differ from the expected multiset"
    if pts is not None and d2 is not None and q is not None:
        assert rows_at_their_d2(q, offsets, pts, d2), f"{who}: some row pairs a point with another point's d2"


def rows_at_their_d2(q, offsets, pts, d2):
    """every returned row pairs a point with ITS d2: calc_dist(query, point) has exactly the returned bits"""
    q = np.asarray(q, np.float32)
    seg = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    dx = q[seg, 0] - pts[:, 0]
    acc = dx * dx
    dy = q[seg, 1] - pts[:, 1]
    acc += dy * dy
    dz = q[seg, 2] - pts[:, 2]
    acc += dz * dz
    return np.array_equal(acc.view(np.uint32), d2.view(np.uint32))


def tree_balls(tree, q, max_dist, k, threads=8):
    """The reference tree's large-k Nearest_Search as (offsets, pts, d2): k must exceed the largest population."""
    tp, td, tc = tree.knn(q, k=k, max_dist=max_dist, threads=threads)
    assert tc.max(initial=0) < k, "k does not exceed the largest ball"
    rows = np.arange(k)[None, :] < tc[:, None]
    return np.concatenate([[0], np.cumsum(tc)]).astype(np.int64), tp[rows], td[rows]


def check_same_balls(offsets, pts, d2, other, who):
    """(offsets, pts, d2) against another such triple (the reference tree's): offsets, d2-bit multisets and point-row multisets."""
    oo, op, od = other
    assert np.array_equal(offsets, oo), f"{who}: counts differ"
    gb, eb = d2.view(np.uint32), od.view(np.uint32)
    assert np.array_equal(gb[_sorted_rows(oo, (gb,))], eb[_sorted_rows(oo, (eb,))]), f"{who}: d2 multisets differ"
    g, e = np.ascontiguousarray(pts).view(np.uint32), np.ascontiguousarray(op).view(np.uint32)
    assert np.array_equal(g[_sorted_rows(oo, (g[:, 0], g[:, 1], g[:, 2]))], e[_sorted_rows(oo, (e[:, 0], e[:, 1], e[:, 2]))]), f"{who}: point multisets differ"
