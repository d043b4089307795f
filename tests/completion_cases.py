"""Inputs that drive a search pass into every k-NN completion path of lii_fit.hip (knn_fallback_wave, complete_one, complete_one_coop,
complete_flagged, k_complete_listed, far_list_trip), and the CPU references the device lists are held to.  No GPU is touched here:
tests/test_completion_cases_host.py asserts the preconditions on the CPU, tests/test_gpu_completion_paths.py runs the cases.

The world is conftest.small_world (24 x 18 x 6 m hall, 0.15 m lattice) WITHOUT the floor patch 0 < x < 9, -4 < y < 4, z < -1.0:
  "win"     that map: the dense cell window is built (row trips of the far pass);
  "hashed"  ... plus one point at (+60, +60, +60) and one at (-60, -60, -60): the window's box would exceed its 64 MiB of entries, none
            is built (column walk over the hashed tables);
  "slab"    "win" plus dense slabs standing in the hole, two brim blocks beside the hall and wall patches that are present two and
            four times (see SlabWorld).
Queries are classified on the CPU tree (oracle.Tree("oracle").knn) at identity pose, where a scan's world point IS its body point:
  F  sure-finished:    d5 < 0.16 m^2 and d5 < d6 - the 3 x 3 x 3 cells prove the list (their guard is at least one cell edge, 0.2025 m^2);
  U  sure-unfinished:  fewer than 5 neighbours within sqrt(5) m, or d5 > 0.81 m^2 ((2 cells)^2, beyond any guard the block can give).
Unfinished-ness is a property of the query and the map alone: a scan of F_N F-queries and u U-queries flags C0 + u.
"""
import numpy as np

FILTER_SIZE_MAP = 0.15
# the library's cell edge (lii_create: 3.0f * map_downsample_size, in float32) and how a coordinate finds its cell (lii_grid.h: cell_of)
CELL = np.float32(3.0) * np.float32(FILTER_SIZE_MAP)
INV_CELL = np.float32(1.0) / CELL
WINDOW_BYTES = 64 << 20   # lii_capi_map.cpp: the window is built if its entries (8 bytes each) fit
MAX_D2 = np.float32(5.0)  # lii_config::max_match_dist2
# lii_device.h / lii_fit.hip / lii_knn.hip (tests/test_completion_cases_host.py reads them from the sources and compares)
K_FLAG_CAP, K_LIST_CAP, K_COMPLETION_BLOCKS_PRE, K_FAR_CAP = 256, 4096, 96, 2048
K_FAR_USE = K_FAR_CAP - 1
SEARCH_TABLE_CHUNKS, SEARCH_LPQ = 64, 4     # CkGeom<4>: MAXCH chunks of LPQ points - what the search pass's table takes
SEARCH_TABLE_POINTS = SEARCH_TABLE_CHUNKS * SEARCH_LPQ

HOLE = ((0.0, 9.0), (-4.0, 4.0), (-np.inf, -1.0))
FLOOR_Z = -1.5
F_N = 3000                # F-queries of every scan
U_MAX = 6000              # the largest U_n
C0 = 0                    # what the F-queries alone flag (asserted first: the U_n = 0 case of test a)
U_EDGES = (0, 1, K_COMPLETION_BLOCKS_PRE, K_COMPLETION_BLOCKS_PRE + 1, K_FLAG_CAP, K_FLAG_CAP + 1, 1500, K_LIST_CAP, K_LIST_CAP + 1, U_MAX)
PLAN_SEQUENCE = (6000, 6000, 6000, 1500, 1500, 10, 10, 10, 1500, 97, 96)
BRUTE_SAMPLE = 300
FAR_POINTS = np.array([[60.0, 60.0, 60.0], [-60.0, -60.0, -60.0]], np.float32)


def cell_of(v):
    """lii_grid.h cell_of in float32: floorf(v * inv_cs)."""
    return np.floor(np.asarray(v, np.float32) * INV_CELL).astype(np.int64)


def in_hole(p):
    (x0, x1), (y0, y1), (_, z1) = HOLE
    return (p[:, 0] > x0) & (p[:, 0] < x1) & (p[:, 1] > y0) & (p[:, 1] < y1) & (p[:, 2] < z1)


def hole_map(small_world):
    _, map_pts = small_world
    m = np.ascontiguousarray(map_pts, np.float32)
    return np.ascontiguousarray(m[~in_hole(m)])


def window_entries(map_pts):
    """Entries of the dense cell window lii_capi_map.cpp would build: the box of the occupied 8 x 8 x 8-cell blocks plus one block of
    margin on every side.  Returns (entries, cells per axis)."""
    b = cell_of(map_pts) >> 3
    dims = [int((b[:, a].max() - b[:, a].min() + 3) * 8) for a in range(3)]
    return dims[0] * dims[1] * dims[2], dims


def has_window(map_pts):
    return window_entries(map_pts)[0] * 8 <= WINDOW_BYTES


def dist2_f32(q, p):
    """KD_TREE::calc_dist in float32, every operation rounded on its own: (dx dx + dy dy) + dz dz."""
    q = np.asarray(q, np.float32)
    p = np.asarray(p, np.float32)
    dx, dy, dz = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1], q[..., 2] - p[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def brute_knn(world_f32, map_f32, sample=None, keep=8):
    """Brute force over the whole map for the queries world_f32[sample]: the `keep` nearest of the points with d^2 <= 5, ascending,
    equal distances in map order.  Returns (points (m, keep, 3), d2 (m, keep) with inf behind the end, count (m,), capped at keep)."""
    q = np.ascontiguousarray(world_f32, np.float32)
    if sample is not None:
        q = q[np.asarray(sample)]
    mp = np.ascontiguousarray(map_f32, np.float32)
    m = len(q)
    pts = np.zeros((m, keep, 3), np.float32)
    d2 = np.full((m, keep), np.inf, np.float32)
    cnt = np.zeros(m, np.int32)
    for a in range(0, m, 64):
        qq = q[a:a + 64]
        d = dist2_f32(qq[:, None, :], mp[None, :, :])
        d = np.where(d <= MAX_D2, d, np.float32(np.inf))
        part = np.sort(np.argpartition(d, keep, axis=1)[:, :keep + 1], axis=1)  # ascending map index, so that the stable sort keeps map order
        dd = np.take_along_axis(d, part, axis=1)
        # (keep + 1 candidates: among equal distances at the partition's edge the partition may have picked any; the first `keep` by
        # (distance, index) of keep + 1 are exact unless the tie runs across the edge, which the callers exclude by their tie rule)
        order = np.argsort(dd, axis=1, kind="stable")[:, :keep]
        idx = np.take_along_axis(part, order, axis=1)
        dk = np.take_along_axis(dd, order, axis=1)
        d2[a:a + 64] = dk
        pts[a:a + 64] = mp[idx]
        cnt[a:a + 64] = np.isfinite(dk).sum(axis=1)
    pts[~np.isfinite(d2)] = 0
    return pts, d2, cnt


class Reference:
    """Tree.knn of a fixed query set on one map, computed once: five lists, the 6th distance (for the 5/6 tie rule) and counts."""

    def __init__(self, tree, queries):
        self.q = np.ascontiguousarray(queries, np.float32)
        self.pts, self.d2, self.cnt = tree.knn(self.q, k=5, threads=4)
        _, d6, c6 = tree.knn(self.q, k=6, threads=4)
        self.d6 = np.where(c6 == 6, d6[:, 5], np.float32(np.inf)).astype(np.float32)
        self.d5 = np.where(self.cnt == 5, self.d2[:, 4], np.float32(np.inf)).astype(np.float32)
        self.tie56 = (self.cnt == 5) & (self.d5 == self.d6)


def classify_F(ref):
    return (ref.cnt == 5) & (ref.d5 < np.float32(0.16)) & (ref.d5 < ref.d6)


def classify_U(ref):
    return (ref.cnt < 5) | (ref.d5 > np.float32(0.81))


def f_candidates(n=6000, seed=101):
    """Floor points outside the hole: x in [-11, -1.5], z noise 0.02."""
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(-11.0, -1.5, n), rng.uniform(-8.0, 8.0, n), FLOOR_Z + rng.normal(0.0, 0.02, n)].astype(np.float32)


def u_candidates(n=12000, seed=102):
    """Points on the floor plane inside the hole."""
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(0.0, 9.0, n), rng.uniform(-4.0, 4.0, n), np.full(n, FLOOR_Z)].astype(np.float32)


class HoleWorld:
    """The hole map in its two variants and the F / U classes (classified on the "win" tree; the two far points of "hashed" are out of
    every query's reach, so the classes are the same there)."""

    def __init__(self, small_world, oracle):
        self.maps = {"win": hole_map(small_world)}
        self.maps["hashed"] = np.ascontiguousarray(np.r_[self.maps["win"], FAR_POINTS])
        self.tree = oracle.Tree("oracle")
        self.tree.build(self.maps["win"])
        fc, uc = f_candidates(), u_candidates()
        self.f_ref_all, self.u_ref_all = Reference(self.tree, fc), Reference(self.tree, uc)
        self.f_ok, self.u_ok = classify_F(self.f_ref_all), classify_U(self.u_ref_all)
        self.F = np.ascontiguousarray(fc[self.f_ok][:F_N])
        self.U = np.ascontiguousarray(uc[self.u_ok][:U_MAX])
        self.queries = np.ascontiguousarray(np.r_[self.F, self.U])  # query id: F first, then U

    def scan(self, u_n):
        """(scan (n, 4) float32 with zero time stamps, ids (n,) into self.queries): F_N F-queries and the first u_n U-queries,
        interleaved by a fixed permutation."""
        ids = np.r_[np.arange(F_N), F_N + np.arange(u_n)]
        ids = ids[np.random.default_rng(7000 + u_n).permutation(len(ids))]
        return np.ascontiguousarray(np.c_[self.queries[ids], np.zeros(len(ids), np.float32)], np.float32), ids

    def is_U(self, ids):
        return ids >= F_N


# ------------------------------------------------------------------------------------------------ the slab world
# Slab A stands in the hole, its near face at x cell 10 (4.5 m): layer 0 holds SLAB_BASE points in every cell of 12 x 11 cells (y, z);
# the cells of layers 0 - 2 within reach of the A-queries' cluster hold SLAB_CORE.  Every trip of a far pass that meets the core lists
# more chunks than the far list holds: those go lane by lane (far_candidates), and the whole ball lists >= 3 x kFarUse chunks.
# Slab B, one layer in mid-air at the hall's other end (x cell -16, nothing else within reach of the B-queries), holds SLAB_B points
# per cell: a row of the window meets ONE of its cells, so a row trip (64 rows) lists at most 64 x 31 = 1984 <= kFarUse chunks - they go
# through the list - and the ball lists more than kFarUse in all: the list is scanned and reset when it is full.
SLAB_BASE, SLAB_CORE, SLAB_B = 84, 184, 124
SLAB_A_X, SLAB_A_Y, SLAB_A_Z = (10, 12), (-6, 5), (-3, 7)       # cell ranges, inclusive
SLAB_B_X, SLAB_B_Y, SLAB_B_Z = (-16, -16), (2, 10), (-1, 7)
A_CENTRE = np.array([3.40, -0.20, 0.95])   # 1.1 m in front of slab A
B_CENTRE = np.array([-8.30, 2.90, 1.55])   # 1.1 m in front of slab B
N_FACING = 64
# The brim blocks: two 8 x 8 x 8-cell blocks beside the hall with nothing around them.  A query in the top cell layer of such a block
# finds no point in its 3 x 3 x 3 cells; its clipped cube is the block's 8 x 8 x 6 cells - 48 rows, ONE row trip - and the cells filled
# here list exactly BRIM chunks in that trip: kFarUse (the far list filled to its last word) and kFarUse + 1 (the smallest trip that goes
# lane by lane).  The query's nearest point is the LAST one listed.
BRIM_BLOCKS = ((5, 0, 0, K_FAR_USE), (5, 3, 0, K_FAR_USE + 1))  # block (x, y, z), chunks
TIE_COPIES = ((2, (-1.0, 1.0)), (4, (3.0, 5.0)))  # wall x = -12: patches y range (z in [0, 2]) present 2 and 4 times
# Queries of each class in a scan of the slab world, beside the F_N F-queries: few enough for one query per completion workgroup (four
# wavefronts together), for one wavefront each in the completion workgroups, and more than those take.  (flagged range of the path)
SLAB_MIXES = {
    "coop": dict(U=0, facing_a=16, facing_b=16, in_slab=16, brim=2, tie=(16, 16)),
    "per_wavefront": dict(U=60, facing_a=32, facing_b=32, in_slab=32, brim=2, tie=(32, 32)),
    "wide": dict(U=300, facing_a=64, facing_b=64, in_slab=64, brim=2, tie=(64, 64)),
}
SLAB_MIX_RANGE = {"coop": (1, K_COMPLETION_BLOCKS_PRE), "per_wavefront": (K_COMPLETION_BLOCKS_PRE + 1, K_FLAG_CAP), "wide": (K_FLAG_CAP + 1, 10 ** 9)}


def _cell_points(rng, ix, iy, iz, n, margin=0.02):
    lo = np.array([ix, iy, iz], np.float64) * float(CELL)
    return (lo + margin + rng.uniform(0.0, 1.0, (n, 3)) * (float(CELL) - 2 * margin)).astype(np.float32)


def cell_gap2(q, cells):
    """Squared distance from q to the boxes of `cells` (m, 3), float64 (the device prunes with a slack of 1e-6: cells within 1e-3 of
    the bound are left out of the guaranteed sums by the callers)."""
    lo = cells.astype(np.float64) * float(CELL)
    g = np.maximum(np.maximum(lo - q, q - (lo + float(CELL))), 0.0)
    return (g * g).sum(axis=1)


class SlabWorld:
    def __init__(self, small_world, oracle):
        rng = np.random.default_rng(303)
        base = hole_map(small_world)
        parts = [base]
        # slab A
        cells_a = np.array([(x, y, z) for x in range(SLAB_A_X[0], SLAB_A_X[1] + 1) for y in range(SLAB_A_Y[0], SLAB_A_Y[1] + 1)
                            for z in range(SLAB_A_Z[0], SLAB_A_Z[1] + 1)])
        core = cell_gap2(A_CENTRE, cells_a) <= 5.0 + 0.5
        for c, is_core in zip(cells_a, core):
            n = SLAB_CORE if is_core else (SLAB_BASE if c[0] == SLAB_A_X[0] else 0)
            if n:
                parts.append(_cell_points(rng, *c, n))
        # slab B
        for y in range(SLAB_B_Y[0], SLAB_B_Y[1] + 1):
            for z in range(SLAB_B_Z[0], SLAB_B_Z[1] + 1):
                parts.append(_cell_points(rng, SLAB_B_X[0], y, z, SLAB_B))
        # brim blocks
        self.brim_queries = []
        for bx, by, bz, chunks in BRIM_BLOCKS:
            pts, q = self._brim_block(rng, bx, by, bz, chunks)
            parts.append(pts)
            self.brim_queries.append(q)
        self.brim_queries = np.array(self.brim_queries, np.float32)
        # wall patches present several times
        self.tie_queries, self.tie_kind = [], []
        for copies, (y0, y1) in TIE_COPIES:
            patch = base[(base[:, 0] < -11.9) & (base[:, 1] > y0) & (base[:, 1] < y1) & (base[:, 2] > 0.0) & (base[:, 2] < 2.0)]
            assert len(patch) > 100, len(patch)
            for _ in range(copies - 1):
                parts.append(patch.copy())
            nq = 64
            self.tie_queries.append(np.c_[np.full(nq, -11.9), rng.uniform(y0 + 0.4, y1 - 0.4, nq), rng.uniform(0.4, 1.6, nq)].astype(np.float32))
            self.tie_kind += [copies] * nq
        self.tie_queries = np.ascontiguousarray(np.concatenate(self.tie_queries))
        self.tie_kind = np.array(self.tie_kind)
        self.map = np.ascontiguousarray(np.concatenate(parts), np.float32)
        self.map_cells = cell_of(self.map)
        self.tree = oracle.Tree("oracle")
        self.tree.build(self.map)
        # the query classes
        self.facing_a = (A_CENTRE + rng.uniform(-0.06, 0.06, (N_FACING, 3))).astype(np.float32)
        self.facing_b = (B_CENTRE + rng.uniform(-0.1, 0.1, (N_FACING, 3))).astype(np.float32)
        ins = np.c_[rng.uniform(4.55, 4.90, 64), rng.uniform(-2.0, 2.0, 64), rng.uniform(-1.0, 3.0, 64)]
        self.in_slab = ins.astype(np.float32)
        uc = u_candidates(1200, seed=104)
        ur = Reference(self.tree, uc)
        self.U = np.ascontiguousarray(uc[classify_U(ur)][:BRUTE_SAMPLE])
        fr_all = f_candidates(4000, seed=105)
        self.F = np.ascontiguousarray(fr_all[classify_F(Reference(self.tree, fr_all))][:F_N])
        groups = [("F", self.F), ("U", self.U), ("facing_a", self.facing_a), ("facing_b", self.facing_b), ("in_slab", self.in_slab),
                  ("brim", self.brim_queries), ("tie", self.tie_queries)]
        self.queries = np.ascontiguousarray(np.concatenate([g for _, g in groups]))
        self.group = np.concatenate([[name] * len(g) for name, g in groups])

    @staticmethod
    def _brim_block(rng, bx, by, bz, chunks):
        """Points of one brim block and its query.  The query sits in cell (4, 3, 7) of the block (top layer, no block above); filled
        are three cells two cells away from it - rows below the last - and, LAST in the trip's order (highest row that holds a point,
        one cell in it), the cell two rows up in y, which holds five points: its second chunk, one point, is the trip's last word and
        the query's fifth neighbour."""
        o = np.array([bx, by, bz]) * 8
        qc = o + np.array([4, 3, 7])
        q = (qc + np.array([0.5, 0.9, 0.5])) * float(CELL)
        near = o + np.array([4, 5, 7])          # row (y = 5, z = 7): the highest filled row; 5 points = 2 chunks
        # the five nearest points of the query, by construction: at 0.5 .. 0.6 m, every other filled cell is farther than 0.9 m
        pn = np.array([(qc[0] + 0.5, near[1] + 0.05 + 0.02 * j, qc[2] + 0.5) for j in range(5)]) * float(CELL)
        rest = chunks - 2
        fill = [o + np.array([1, 3, 7]), o + np.array([7, 3, 7]), o + np.array([4, 0, 7])]   # gaps of 2 cells: 0.9 m and more
        per = [rest // 3, rest // 3, rest - 2 * (rest // 3)]
        pts = [pn.astype(np.float32)]
        for c, ch in zip(fill, per):
            pts.append(_cell_points(rng, *c, 4 * ch))   # full chunks
        return np.concatenate(pts), q.astype(np.float32)

    def cell_counts(self):
        if not hasattr(self, "_cells"):
            self._cells = np.unique(self.map_cells, axis=0, return_counts=True)
        return self._cells

    def ball_chunks(self, q, keys=None, counts=None):
        """Sum of ceil(n_cell / 4) over the cells the far pass of a query with an empty inner list must list: box within sqrt(5) m (less
        1e-3 of slack), outside the 3 x 3 x 3 cells, inside the 27 blocks around the query."""
        if keys is None:
            keys, counts = self.cell_counts()
        qc = cell_of(q)
        inner = (np.abs(keys - qc) <= 1).all(axis=1)
        blocks = (np.abs((keys >> 3) - (qc >> 3)) <= 1).all(axis=1)
        ok = (cell_gap2(np.asarray(q, np.float64), keys) <= 5.0 - 1e-3) & ~inner & blocks
        return int(((counts[ok] + 3) // 4).sum())

    def row_trip_totals(self, q, bound=5.0):
        """Chunks that each trip of the windowed far pass of ONE wavefront (knn_fallback_wave, rows_ok: 64 rows of the clipped cube per
        trip, 14 cells of a row) hands to far_list_trip, for a query whose far pass is bounded by `bound` (5: an empty inner list).
        A model in float64 without the device's slack of 1e-6: a cell whose box touches the ball's surface may differ."""
        if not hasattr(self, "_table"):
            keys, counts = self.cell_counts()
            self._table = {tuple(k): int(c) for k, c in zip(keys.tolist(), counts.tolist())}
            self._blocks = set(map(tuple, np.unique(keys >> 3, axis=0).tolist()))
        q64 = np.asarray(q, np.float64)
        cs = float(CELL)
        qc = cell_of(q)
        b0 = qc >> 3
        r1 = np.sqrt(bound)
        lo, hi = cell_of(q64 - r1), cell_of(q64 + r1)
        around = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (b0[0] + x, b0[1] + y, b0[2] + z) in self._blocks]
        for a in range(3):  # the cube is clipped to the block layers that exist among the 27 around the query
            layers = sorted({d[a] for d in around})
            lo[a] = max(lo[a], (b0[a] + layers[0]) * 8)
            hi[a] = min(hi[a], (b0[a] + layers[-1]) * 8 + 7)
        nx, ny, nz = [int(max(hi[a] - lo[a] + 1, 0)) for a in range(3)]
        xs0 = int(lo[0]) - (int(lo[0]) & 1)  # (the window's origin is a multiple of eight cells)
        trips = []
        for r0 in range(0, ny * nz, 64):
            for xs in range(xs0, int(hi[0]) + 1, 14):
                total = 0
                for r in range(r0, min(r0 + 64, ny * nz)):
                    iy, iz = int(lo[1]) + r % ny, int(lo[2]) + r // ny
                    for ix in range(max(xs, int(lo[0])), min(xs + 14, int(hi[0]) + 1)):
                        n = self._table.get((ix, iy, iz), 0)
                        if not n or (abs(ix - qc[0]) <= 1 and abs(iy - qc[1]) <= 1 and abs(iz - qc[2]) <= 1):
                            continue
                        g2 = 0.0
                        for v, i in zip(q64, (ix, iy, iz)):
                            g = max(i * cs - v, v - (i + 1) * cs, 0.0)
                            g2 += g * g
                        if g2 <= bound:
                            total += (n + 3) // 4
                trips.append(total)
        return trips

    def points_in_27(self, q):
        qc = cell_of(q)
        return int((np.abs(self.map_cells - qc) <= 1).all(axis=1).sum())

    def chunks_in_nearest_8(self, q):
        """Chunks of the 2 x 2 x 2 cells round 1 of the search pass looks up (own cell + the neighbour on the nearer side per axis)."""
        q = np.asarray(q, np.float32)
        qc = cell_of(q)
        f = q - qc.astype(np.float32) * CELL
        o = np.where(f < np.float32(0.5) * CELL, -1, 1)
        keys, counts = self.cell_counts()
        total = 0
        for c in range(8):
            cell = qc + np.array([(c & 1) * o[0], ((c >> 1) & 1) * o[1], ((c >> 2) & 1) * o[2]])
            hit = (keys == cell).all(axis=1)
            if hit.any():
                total += int((counts[hit][0] + 3) // 4)
        return total

    def scan(self, mix):
        """(scan, ids into self.queries, flagged queries that are sure, at most) for one of SLAB_MIXES.  Sure: the U, slab-facing, in-slab
        and brim queries and the queries of the four-fold patch (their 5th distance is their 7th: ambiguous); the two-fold patch's are
        flagged only if their 7th distance agrees with the 5th in the bits the search pass keeps."""
        m = SLAB_MIXES[mix]
        take = [np.flatnonzero(self.group == "F")]
        for name in ("U", "facing_a", "facing_b", "in_slab", "brim"):
            take.append(np.flatnonzero(self.group == name)[:m[name]])
        tie = np.flatnonzero(self.group == "tie")
        for copies, k in zip((2, 4), m["tie"]):
            take.append(tie[self.tie_kind == copies][:k])
        ids = np.concatenate(take)
        ids = ids[np.random.default_rng(7300 + len(ids)).permutation(len(ids))]
        sure = sum(m[name] for name in ("U", "facing_a", "facing_b", "in_slab", "brim")) + m["tie"][1]
        return np.ascontiguousarray(np.c_[self.queries[ids], np.zeros(len(ids), np.float32)], np.float32), ids, sure, sure + m["tie"][0]


def lists_agree(world, nb, cnt, ref_pts, ref_d2, ref_cnt, tie56, map_set):
    """The comparison of check_lists, as data: device lists (nb (n, 5, 3), cnt) against a reference (points, distances, counts) for the
    same world points.  Counts must agree for every query; the first cnt entries must be bit-equal in points and in the float32
    distances recomputed from them, except where the reference has a 5/6 tie (tie56) - there the distances must be bit-equal and every
    point a member of the map (map_set: point_set).  Returns the problems found, as strings (none: the lists agree)."""
    problems = []
    if not np.array_equal(cnt, ref_cnt):
        bad = np.flatnonzero(cnt != ref_cnt)
        problems.append(f"count differs at {len(bad)} queries, first {bad[:5].tolist()}: device {cnt[bad[:5]].tolist()} reference {ref_cnt[bad[:5]].tolist()}")
        return problems
    valid = np.arange(5)[None, :] < cnt[:, None]
    dev_d = dist2_f32(world[:, None, :], nb)
    same_pts = (nb.view(np.uint32) == ref_pts.view(np.uint32)).all(axis=2)
    same_d = dev_d.view(np.uint32) == np.ascontiguousarray(ref_d2[:, :5], np.float32).view(np.uint32)
    strict = ~tie56
    bad = strict & ((~same_pts | ~same_d) & valid).any(axis=1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        problems.append(f"{int(bad.sum())} lists differ, first query {i}: device {nb[i].tolist()} reference {ref_pts[i].tolist()}")
    loose = tie56
    bad_d = loose & (~same_d & valid).any(axis=1)
    if bad_d.any():
        problems.append(f"{int(bad_d.sum())} tied lists differ in their distances, first query {int(np.flatnonzero(bad_d)[0])}")
    if loose.any():
        rows = np.ascontiguousarray(nb[loose].reshape(-1, 3))
        if not all(r.tobytes() in map_set for r in rows):
            problems.append("a tied list holds a point that is not in the map")
    return problems


def point_set(map_pts):
    """The map's points as a set of their 12 bytes."""
    raw = np.ascontiguousarray(map_pts, np.float32).tobytes()
    return {raw[i:i + 12] for i in range(0, len(raw), 12)}
