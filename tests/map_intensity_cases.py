"""Case builders of the map-intensity tests (tests/test_gpu_map_intensity.py) and their self-checks (tests/test_map_intensity_cases.py).

Expected intensities never come from the library.  The reference tree moves whole points (Add_Points keeps downsample_result,
include/ikd-Tree/ikd_Tree.cpp:381-456), so a stored point's intensity is a function of its xyz bits: every cloud here has pairwise distinct
(x, y, z) bit triples, and the expectation for any row the library returns is a lookup of its triple in the inputs (`Table`).  Everything is
compared bit for bit (uint32 views)."""
import numpy as np

DS = 0.2  # the down-sample box of the fold cases (filter_size_map)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_distinct_triples(*clouds):
    """The (x, y, z) bit triples of all the clouds together are pairwise distinct."""
    xyz = np.concatenate([np.ascontiguousarray(c, np.float32)[:, :3] for c in clouds])
    assert len(np.unique(bits(xyz), axis=0)) == len(xyz), "a cloud of the test holds an (x, y, z) triple twice"


def with_intensity(xyz, first=1):
    """(n, 4): xyz and an intensity of its own per point - k + 0.25 for the k-th point counted from `first`: exact in float32 up to 2^21,
    never 0 (what a point without intensity carries), distinct across the clouds of a test when `first` continues the count."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    assert first >= 1 and first + len(xyz) < (1 << 21)
    w = (np.arange(first, first + len(xyz), dtype=np.float64) + 0.25).astype(np.float32)
    return np.ascontiguousarray(np.c_[xyz, w], np.float32)


def distinct_cloud(rng, n, lo=-10.0, hi=10.0, first=1):
    """n' <= n points (x, y, z, intensity) with distinct triples and no zero coordinate, in random order."""
    p = np.unique(rng.uniform(lo, hi, (n, 3)).astype(np.float32), axis=0)
    p = p[(p != 0).all(axis=1)]
    return with_intensity(p[rng.permutation(len(p))], first)


def as_xyzinormal(xyzi):
    """The same points as 48-byte pcl::PointXYZINormal records (12 floats: x y z pad | normal xyz pad | intensity curvature pad pad), the other
    words filled with values that must not be mistaken for the intensity."""
    xyzi = np.ascontiguousarray(xyzi, np.float32)
    rec = np.full((len(xyzi), 12), -7.5, np.float32)
    rec[:, :3] = xyzi[:, :3]
    rec[:, 8] = xyzi[:, 3]
    return rec


class Table:
    """xyz bit triple -> intensity bits, over every input a map has been given."""

    def __init__(self, *clouds):
        self.d = {}
        for c in clouds:
            self.add(c)

    def add(self, xyzi):
        xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
        b = bits(xyzi)
        for r in b:
            k = r[:3].tobytes()
            assert k not in self.d, "an (x, y, z) triple given twice"
            self.d[k] = int(r[3])

    def expect(self, rows):
        """The uint32 intensity bits the rows (m, >= 3; xyz first) must carry."""
        b = bits(np.ascontiguousarray(rows, np.float32)[:, :3])
        return np.array([self.d[r.tobytes()] for r in b], np.uint32)

    def check(self, rows_xyzi):
        rows_xyzi = np.ascontiguousarray(rows_xyzi, np.float32).reshape(-1, 4)
        got = bits(rows_xyzi)[:, 3]
        want = self.expect(rows_xyzi)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{bad.size} of {len(got)} rows carry another intensity than their input point (first: row {bad[0]}, " \
                              f"{rows_xyzi[bad[0]]}, expected bits {want[bad[0]]:#x})"


def same_rows_as_set(a, b):
    """Two arrays of rows hold the same multiset of rows, bit for bit."""
    a, b = bits(a), bits(b)
    if a.shape != b.shape:
        return False
    a = a[np.lexsort(a.T[::-1])]
    b = b[np.lexsort(b.T[::-1])]
    return np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ the fold (Add_Points, down-sampling on)
def _voxel_points(rng, voxel, radii, ds):
    """One point per radius at that distance (in units of ds) from the voxel's centre, well inside the box (|offset| <= 0.4 ds an axis)."""
    c = (np.asarray(voxel, np.float64) + 0.5) * ds
    out = []
    for r in radii:
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        out.append(c + u * r * ds)
    return np.array(out, np.float64).reshape(-1, 3)


def voxel_of(xyz, ds):
    """floor(x / ds) in float arithmetic, as Add_Points forms it (ikd_Tree.cpp:390-395)."""
    xyz = np.ascontiguousarray(xyz, np.float32)[:, :3]
    return np.floor(xyz / np.float32(ds)).astype(np.int64)


def centre_d2(xyz, ds):
    """Squared distance to the centre of the point's own down-sample box (float64: the cases keep the distances of a voxel far apart)."""
    xyz = np.ascontiguousarray(xyz, np.float32)[:, :3].astype(np.float64)
    v = np.floor(xyz / ds)
    return (((xyz - (v + 0.5) * ds)) ** 2).sum(axis=1)


def fold_case(seed=5, ds=DS, origin=(40, -30, 7)):
    """A map (`stored`, built without down-sampling) and one batch (`batch`, added WITH down-sampling) whose voxels cover the fold's paths:
         kind            stored points in the box     batch points in the voxel
         "empty"         0                            1, 3, 8, 9, 20  (9 and 20 leave the eight-lane shuffle for the replay from memory)
         "stored_wins"   1, the closest of all        1, 3, 9
         "batch_wins"    1                            1, 3, 9, one of them the closest of all
         "multi_stored"  3 (all but the survivor go)  2: once a stored point is the closest, once a batch point
       plus stored points in voxels the batch does not touch (they stay, several a voxel).  The radii come from one strictly increasing pool,
       so no two points of the case are equally far from a centre.  Returns a dict: stored, batch (n, 4 each), ds, voxels: list of (kind,
       voxel, n_stored, n_batch), survivors: (m, 4) - the map after the batch, by the rule "per touched box the point closest to the centre,
       every other stored point of the box gone; untouched points stay" (Add_Points, ikd_Tree.cpp:381-456)."""
    rng = np.random.default_rng(seed)
    plan = [("empty", 0, b, None) for b in (1, 3, 8, 9, 20)]
    plan += [("stored_wins", 1, b, "stored") for b in (1, 3, 9)]
    plan += [("batch_wins", 1, b, "batch") for b in (1, 3, 9)]
    plan += [("multi_stored", 3, 2, "stored"), ("multi_stored", 3, 2, "batch")]
    n_pts = sum(s + b for _, s, b, _ in plan)
    pool = list(np.linspace(0.04, 0.38, n_pts))  # radii in units of ds; neighbouring radii differ by > 0.005 ds
    stored, batch, voxels = [], [], []
    for j, (kind, ns, nb, winner) in enumerate(plan):
        voxel = (origin[0] + 2 * j, origin[1] + (j % 3), origin[2] - (j % 2))  # apart from each other: no box holds another voxel's points
        radii = sorted(pool.pop(0) for _ in range(ns + nb))
        if winner == "stored":  # (the smallest radius goes to the side that is to win, the others are dealt out at random)
            who = ["s"] + list(rng.permutation(["s"] * (ns - 1) + ["b"] * nb))
        elif winner == "batch":
            who = ["b"] + list(rng.permutation(["s"] * ns + ["b"] * (nb - 1)))
        else:
            who = ["b"] * nb
        pts = _voxel_points(rng, voxel, radii, ds)
        stored += [p for p, w in zip(pts, who) if w == "s"]
        b_here = [p for p, w in zip(pts, who) if w == "b"]
        batch += [b_here[i] for i in rng.permutation(len(b_here))]  # the closest batch point is not always the first
        voxels.append((kind, voxel, ns, nb))
    # stored points nobody touches: three in one voxel, one each in two others
    for voxel, k in (((origin[0] - 4, origin[1], origin[2]), 3), ((origin[0] - 6, origin[1], origin[2]), 1), ((origin[0] - 8, origin[1] + 1, origin[2]), 1)):
        stored += list(_voxel_points(rng, voxel, np.linspace(0.1, 0.3, k), ds))
    stored = with_intensity(np.array(stored, np.float32), first=1)
    batch = np.array(batch, np.float32)
    batch = with_intensity(batch[rng.permutation(len(batch))], first=1 + len(stored))  # the voxels' points interleaved in the batch
    # the survivors, by the rule
    allp = np.concatenate([stored, batch])
    is_batch = np.r_[np.zeros(len(stored), bool), np.ones(len(batch), bool)]
    vox = voxel_of(allp, ds)
    d2 = centre_d2(allp, ds)
    keep = np.ones(len(allp), bool)
    touched = {tuple(v) for v in vox[is_batch]}
    for v in touched:
        m = np.flatnonzero((vox == np.array(v)).all(axis=1))
        keep[m] = False
        keep[m[np.argmin(d2[m])]] = True
    return {"stored": stored, "batch": batch, "ds": ds, "voxels": voxels, "survivors": allp[keep]}


def check_fold_case(case):
    """The case is what fold_case's text says (the self-check of tests/test_map_intensity_cases.py; the GPU test calls it too)."""
    stored, batch, ds = case["stored"], case["batch"], case["ds"]
    assert_distinct_triples(stored, batch)
    assert len(np.unique(bits(np.r_[stored[:, 3], batch[:, 3]]))) == len(stored) + len(batch) and (np.r_[stored[:, 3], batch[:, 3]] != 0).all()
    vs, vb = voxel_of(stored, ds), voxel_of(batch, ds)
    ds2, db2 = centre_d2(stored, ds), centre_d2(batch, ds)
    # every point is well inside its box (the float floor cannot put it elsewhere) and no two distances of the case are close
    for p in (stored, batch):
        f = p[:, :3].astype(np.float64) / ds
        assert (np.abs(f - np.floor(f) - 0.5) < 0.45).all()
    seen = {}
    for kind, voxel, ns, nb in case["voxels"]:
        ms, mb = (vs == np.array(voxel)).all(axis=1), (vb == np.array(voxel)).all(axis=1)
        assert ms.sum() == ns and mb.sum() == nb, (kind, voxel, int(ms.sum()), int(mb.sum()))
        d = np.sort(np.r_[ds2[ms], db2[mb]])
        assert (np.diff(d) > 1e-6 * ds * ds).all(), "two points of a voxel are equally far from its centre"
        best_batch = db2[mb].min()
        if kind == "stored_wins":
            assert ds2[ms].min() < best_batch
        if kind == "batch_wins":
            assert best_batch < ds2[ms].min()
        if kind in ("batch_wins", "empty") and nb > 1:
            seen.setdefault("closest_not_first", []).append(int(np.argmin(db2[mb])) != 0)
        seen.setdefault(kind, []).append(nb)
    assert sorted(seen["empty"]) == [1, 3, 8, 9, 20] and sorted(seen["stored_wins"]) == [1, 3, 9] and sorted(seen["batch_wins"]) == [1, 3, 9]
    assert len(seen["multi_stored"]) == 2 and any(seen["closest_not_first"])
    # both outcomes of a box with several stored points
    outcomes = set()
    for kind, voxel, ns, nb in case["voxels"]:
        if kind == "multi_stored":
            ms, mb = (vs == np.array(voxel)).all(axis=1), (vb == np.array(voxel)).all(axis=1)
            outcomes.add(bool(ds2[ms].min() < db2[mb].min()))
    assert outcomes == {True, False}
    # untouched stored points: a voxel with three of them
    touched = {tuple(v) for v in vb}
    un = [tuple(v) for v in vs if tuple(v) not in touched]
    assert len(un) == 5 and max(un.count(v) for v in set(un)) == 3
    # the survivors: one per touched voxel, plus the untouched
    sv = voxel_of(case["survivors"], ds)
    for v in touched:
        assert (sv == np.array(v)).all(axis=1).sum() == 1
    assert len(case["survivors"]) == len(touched) + 5


def growth_batches(seed=9, cell=(150, 150, 3), cell_size=0.6, n=40):
    """40 points of ONE grid cell (edge cell_size, map_cell_size of the handle), for inserts without down-sampling: a cell that outgrows its
    slack and moves to the tail of the point array."""
    rng = np.random.default_rng(seed)
    lo = np.asarray(cell, np.float64) * cell_size
    p = (lo + rng.uniform(0.1, 0.9, (4 * n, 3)) * cell_size).astype(np.float32)
    p = np.unique(p, axis=0)[:n]
    assert len(p) == n
    return with_intensity(p[rng.permutation(n)], first=1000)


def check_growth_batches(p, cell=(150, 150, 3), cell_size=0.6):
    assert_distinct_triples(p)
    c = np.floor(p[:, :3] * np.float32(1.0 / cell_size)).astype(np.int64)  # floorf(p * inv_cs), as the grid forms it
    assert (c == np.array(cell)).all(), "the points do not share one grid cell"
    assert len(p) == 40 and (p[:, 3] != 0).all()
