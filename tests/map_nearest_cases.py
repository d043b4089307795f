"""What the Nearest_Search tests share (test_map_nearest_ref.py on the CPU, test_gpu_map_nearest.py on the device): the seeded query
set, the float32 brute force it is held to, and the comparison of a (pts, d2, count) answer with it.

The brute force is the reference's calc_dist written out - dx*dx + dy*dy + dz*dz in float32, left to right, no FMA (numpy rounds every
operation) - over all map points; per query it keeps the KEEP smallest d2 <= D2_MAX with their map indices, ascending in (d2, index),
ONCE per (map, query set).  Every (k, max_dist) case is cut out of that."""
import numpy as np

KEEP = 65       # one more than the largest k: the entry behind a full list tells whether its edge is tied
D2_MAX = 30.0   # the largest max_dist of the cases
KS = (1, 5, 32, 64)
MAX_DISTS = (1.0, 5.0, 30.0)
CASES = [(k, md) for k in KS for md in MAX_DISTS]
TIED_SHARE_MAX = 0.01  # of the queries of a case may have two equal d2 in their list or at its edge (measured on this input: <= 0.05 %)


def query_set(hall, map_pts, n=2000, seed=41):
    """n points: map points themselves (d2 = 0), points on the surfaces, inside the hall, up to 8 m outside it, one at 1e7 m and one
    with a NaN coordinate.  With max_dist 1 the points in the free space have an empty or a short result, the far ones an empty one."""
    rng = np.random.default_rng(seed)
    n_self, n_surf, n_in = n // 4, n // 4, n // 4
    n_out = n - n_self - n_surf - n_in - 2
    lo, hi = np.asarray(hall.lo, np.float64), np.asarray(hall.hi, np.float64)
    q = np.concatenate([
        map_pts[rng.choice(len(map_pts), n_self, replace=False)].astype(np.float64),
        map_pts[rng.choice(len(map_pts), n_surf, replace=False)] + rng.normal(0, 0.05, (n_surf, 3)),
        rng.uniform(lo, hi, (n_in, 3)),
        rng.uniform(lo - 8.0, hi + 8.0, (n_out, 3)),
        [[1e7, -3.0, 2.0]],
        [[1.0, np.nan, 0.5]],
    ]).astype(np.float32)
    assert len(q) == n
    return q


def d2_f32(q, pts):
    """(len(q), len(pts)) float32: calc_dist of every pair."""
    q = np.asarray(q, np.float32)
    pts = np.asarray(pts, np.float32)
    dx = q[:, None, 0] - pts[None, :, 0]
    acc = dx * dx
    dy = q[:, None, 1] - pts[None, :, 1]
    acc += dy * dy
    dz = q[:, None, 2] - pts[None, :, 2]
    acc += dz * dz
    return acc


class Brute:
    """d2[i, j], idx[i, j]: the j-th nearest map point of query i among those with d2 <= d2_max (j < m[i] <= keep), ascending in (d2, index)."""

    def __init__(self, q, pts, keep=KEEP, d2_max=D2_MAX, chunk=64):
        self.q = np.asarray(q, np.float32)
        self.pts = np.ascontiguousarray(pts, np.float32)
        n = len(self.q)
        keep = min(keep, len(self.pts))
        self.d2 = np.full((n, keep), np.inf, np.float32)
        self.idx = np.zeros((n, keep), np.int64)
        self.m = np.zeros(n, np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            for a in range(0, n, chunk):
                d = d2_f32(self.q[a:a + chunk], self.pts)
                d[~(d <= np.float32(d2_max))] = np.inf  # (a NaN query: nothing qualifies)
                part = np.argpartition(d, keep - 1, axis=1)[:, :keep] if keep < d.shape[1] else np.tile(np.arange(d.shape[1]), (len(d), 1))
                dp = np.take_along_axis(d, part, axis=1)
                # every entry equal to the largest kept d2 must compete by index: argpartition picks among equals arbitrarily
                for r in range(len(d)):
                    edge = dp[r].max()
                    if np.isfinite(edge) and np.count_nonzero(d[r] == edge) > np.count_nonzero(dp[r] == edge):
                        cand = np.flatnonzero(d[r] <= edge)
                        cand = cand[np.lexsort((cand, d[r, cand]))][:keep]
                        part[r], dp[r] = cand, d[r, cand]
                order = np.lexsort((part, dp), axis=1)
                self.idx[a:a + chunk] = np.take_along_axis(part, order, axis=1)
                self.d2[a:a + chunk] = np.take_along_axis(dp, order, axis=1)
        self.m = np.isfinite(self.d2).sum(axis=1)

    def case(self, k, max_dist):
        """count (n,), d2 (n, k) and idx (n, k) (valid below count), tied (n,): two equal d2 inside the list or across its end."""
        ok = self.d2.astype(np.float64) <= float(max_dist)  # (float d2 against the double max_dist, as Search compares)
        m = ok.sum(axis=1)
        count = np.minimum(m, k)
        kk = min(k + 1, self.d2.shape[1])
        d = np.where(ok, self.d2, np.inf)[:, :kk]
        j = np.arange(kk - 1)[None, :]
        # the pair (j, j + 1) matters when j is in the list and j + 1 qualifies (inside the list, or the first one left out)
        pair = (d[:, :-1] == d[:, 1:]) & np.isfinite(d[:, 1:]) & (j < count[:, None])
        w = min(k, self.d2.shape[1])  # (a map of fewer than k points)
        d_out = np.full((len(m), k), np.inf, np.float32)
        i_out = np.zeros((len(m), k), np.int64)
        d_out[:, :w], i_out[:, :w] = self.d2[:, :w], self.idx[:, :w]
        return count, d_out, i_out, pair.any(axis=1)


_cache = {}


def small_world_brute(small_world):
    """The 2 000-query set over the suite's hall map and its brute force, computed once per session."""
    if "sw" not in _cache:
        hall, map_pts = small_world
        map_pts = np.ascontiguousarray(map_pts, np.float32)
        q = query_set(hall, map_pts)
        _cache["sw"] = (q, Brute(q, map_pts))
    return _cache["sw"]


def check_answer(brute, k, max_dist, pts, d2, count, who, pad=0.0, tied_share_max=TIED_SHARE_MAX):
    """Holds an answer to the brute force: counts equal, d2[:count] bit-equal for EVERY query, points equal wherever no two d2 in the
    list or at its edge are equal (such queries: at most tied_share_max of all; there every returned point must be a map point at
    the stated d2), the rows from count on equal to `pad`.  Prints the figures before it asserts.  Returns the share of tied queries."""
    count = np.asarray(count)
    bc, bd, bi, tied = brute.case(k, max_dist)
    n = len(count)
    rows = np.arange(k)[None, :] < bc[:, None]
    share = float(tied.mean()) if n else 0.0
    n_cnt = int(np.count_nonzero(count != bc))
    same_d2 = np.where(rows, d2.view(np.uint32) == bd.view(np.uint32), True)
    exp_pts = brute.pts[bi]
    same_pts = np.where(rows[:, :, None], pts == exp_pts, True).all(axis=2)
    print(f"{who} k={k} max_dist={max_dist}: {n} queries, counts differ {n_cnt}, d2 rows differ {int((~same_d2).sum())}, "
          f"tied queries {int(tied.sum())} ({100 * share:.3f} %), point rows differ outside them {int((~same_pts[~tied]).sum())}")
    assert n_cnt == 0, f"{who}: {n_cnt} counts differ from the brute force"
    assert same_d2.all(), f"{who}: d2 differs from the brute force in {int((~same_d2).sum())} rows"
    assert share <= tied_share_max, f"{who}: {share:.4f} of the queries have equal distances"
    assert same_pts[~tied].all(), f"{who}: points differ from the brute force where no distances are equal"
    # a tied list: every point is a map point at exactly the stated d2
    for i in np.flatnonzero(tied & ~same_pts.all(axis=1)):
        for j in range(bc[i]):
            hit = np.flatnonzero((brute.pts == pts[i, j]).all(axis=1))
            assert len(hit), f"{who}: query {i} row {j} is not a map point"
            assert d2_f32(brute.q[i:i + 1], brute.pts[hit[:1]])[0, 0].view(np.uint32) == d2[i, j].view(np.uint32)
    if np.isinf(pad):
        assert np.isinf(d2[~rows]).all() and not pts[~rows].any(), f"{who}: rows past count"
    else:
        assert not d2[~rows].any() and not pts[~rows].any(), f"{who}: rows past count are not zero"
    return share
