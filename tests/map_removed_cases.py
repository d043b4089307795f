"""What the history-buffer tests share (test_map_removed_abi.py on the CPU, test_gpu_map_removed.py on the device): a map of a few thousand
points cut out of the suite's hall, the box sets of the cases, the numpy brute force of Delete_Point_Boxes' rule - min <= p < max on every
axis, float32 against float32 - and the comparison of point MULTISETS by their float bits.  Nothing here carries a tolerance.

The map: every tenth point of conftest.small_world's 0.15 m lattice, 100 points crowded into ONE grid cell (a lane of the squeeze then
drops more than 64 points of one cell), and points placed exactly on the faces of the `faces` box.  The library's grid at filter_size_map
0.15 has cells of 0.45 m and blocks of 8 x 8 x 8 cells = 3.6 m: the `swallow` box (13 x 12 x 4.6 m) contains whole blocks - the path of
the moving local map that sets tombstones without reading a point."""
import numpy as np

CELL = 0.45
FILTER_SIZE_MAP = 0.15  # ... of the Registrar the device tests create: the cell edge is three times that
CROWD_CELL = (2, -3, 2)  # grid cell of the crowded points: [0.9, 1.35) x [-1.35, -0.9) x [0.9, 1.35)
N_CROWD = 100

FACES_BOX = np.array([-7.5, -4.0, -1.0, 4.5, 2.5, 3.0], np.float32)

# name -> (n, 6) float32 boxes: min xyz, max xyz
BOX_SETS = {
    # one box; the map holds points exactly on its six faces
    "faces": np.array([FACES_BOX], np.float32),
    # two boxes that overlap in a slab
    "overlap2": np.array([[-12.5, -9.5, -2.0, -2.0, 0.0, 5.0], [-6.0, -3.0, -2.0, 1.0, 9.5, 5.0]], np.float32),
    # three, as the boxes of a cube move along x, y and z overlap at a corner
    "overlap3": np.array([[-13.0, -10.0, -2.0, -8.0, 10.0, 5.0], [-13.0, -10.0, -2.0, 13.0, -5.0, 5.0], [-13.0, -10.0, -2.0, 13.0, 10.0, -1.0]], np.float32),
    # an empty box (min = max on x), one with min > max, one that touches nothing, and one that does
    "empty_and_miss": np.array([[1.0, -9.5, -2.0, 1.0, 9.5, 5.0], [3.0, 3.0, 3.0, 2.0, 2.0, 2.0], [40.0, 40.0, 40.0, 45.0, 45.0, 45.0],
                                [8.0, -9.5, -2.0, 12.5, -6.0, 5.0]], np.float32),
    # 13 x 12 x 4.6 m: swallows whole 3.6 m blocks (x [-7.2, 3.6), y [-10.8, -3.6), z [0, 3.6)), the wall y = -9 among them
    "swallow": np.array([[-8.0, -11.0, -0.5, 5.0, 1.0, 4.1]], np.float32),
    # a small box around the crowded cell
    "crowded": np.array([[0.5, -1.8, 0.5, 1.8, -0.5, 1.8]], np.float32),
}
CASES = tuple(BOX_SETS)

_cache = {}


def rows_sorted(a):
    """The rows of an (n, 3) float32 array as uint32 bits, sorted: two arrays hold the same multiset iff these are equal."""
    u = np.ascontiguousarray(a, np.float32).reshape(-1, 3).view(np.uint32)
    return u[np.lexsort((u[:, 2], u[:, 1], u[:, 0]))]


def same_multiset(a, b):
    ra, rb = rows_sorted(a), rows_sorted(b)
    return ra.shape == rb.shape and bool(np.array_equal(ra, rb))


def in_boxes(p, boxes):
    """(len(p),) bool: min <= p < max on every axis for at least one box (ikd_Tree.cpp:970-985, float against float)."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    dead = np.zeros(len(p), bool)
    for b in np.ascontiguousarray(boxes, np.float32).reshape(-1, 6):
        dead |= ((b[:3] <= p) & (p < b[3:])).all(axis=1)
    return dead


def swallowed_blocks(p, box, cell=CELL):
    """Occupied 8 x 8 x 8 blocks of the grid whose whole extent lies inside `box` with a margin of a hundredth of a cell."""
    blk = np.unique(np.floor(np.asarray(p, np.float32) / np.float32(cell)).astype(np.int64) >> 3, axis=0)
    lo = blk * 8 * cell - 0.01 * cell
    hi = (blk + 1) * 8 * cell + 0.01 * cell
    return int(((box[:3] <= lo) & (hi < box[3:])).all(axis=1).sum())


def world(small_world):
    """(map points (n, 3) float32, {case: (boxes, removed mask)}), made once per session."""
    if "w" in _cache:
        return _cache["w"]
    _, map_pts = small_world
    rng = np.random.default_rng(23)
    base = np.ascontiguousarray(map_pts, np.float32)[::10]
    c0 = np.array(CROWD_CELL, np.float64) * CELL
    crowd = rng.uniform(c0 + 0.02, c0 + CELL - 0.02, (N_CROWD, 3)).astype(np.float32)
    faces = []
    b = FACES_BOX
    for a in range(3):
        for face in (b[a], b[3 + a]):
            q = rng.uniform(b[:3] + 0.1, b[3:] - 0.1, (15, 3)).astype(np.float32)
            q[:, a] = face
            faces.append(q)
    pts = np.ascontiguousarray(np.concatenate([base, crowd, np.concatenate(faces)]), np.float32)
    cases = {name: (boxes, in_boxes(pts, boxes)) for name, boxes in BOX_SETS.items()}
    # ---- the cases hold what they are meant to hold
    assert 3000 < len(pts) < 12000
    cell = np.floor(crowd / np.float32(CELL)).astype(int)
    assert (cell == np.array(CROWD_CELL)).all()
    dead = cases["faces"][1]
    on_min = np.zeros(len(pts), bool)
    on_max = np.zeros(len(pts), bool)
    inside_closed = ((b[:3] <= pts) & (pts <= b[3:])).all(axis=1)
    for a in range(3):
        on_min |= inside_closed & (pts[:, a] == b[a])
        on_max |= inside_closed & (pts[:, a] == b[3 + a])
    assert on_min.sum() >= 45 and on_max.sum() >= 45
    assert dead[on_min & ~on_max].all() and not dead[on_max].any()  # the min faces go, the max faces stay
    for name in ("overlap2", "overlap3"):
        boxes = BOX_SETS[name]
        hits = sum(in_boxes(pts, boxes[i:i + 1]).astype(int) for i in range(len(boxes)))
        assert (hits >= 2).sum() > 10, name  # points inside more than one box: collected once
        if name == "overlap3":
            assert (hits == 3).sum() > 0
    boxes = BOX_SETS["empty_and_miss"]
    assert not in_boxes(pts, boxes[:3]).any() and in_boxes(pts, boxes[3:]).sum() > 10
    assert swallowed_blocks(pts, BOX_SETS["swallow"][0]) >= 1
    crowd_dead = cases["crowded"][1]
    assert crowd_dead[len(base):len(base) + N_CROWD].all() and N_CROWD > 64
    counts = {name: int(m.sum()) for name, (_, m) in cases.items()}
    assert all(c > 0 for c in counts.values())
    assert sum(c % 64 != 0 for c in counts.values()) >= 4, counts  # counts that do not fill the last wavefront's reservation
    _cache["w"] = (pts, cases)
    return _cache["w"]
