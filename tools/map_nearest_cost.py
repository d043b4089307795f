#!/usr/bin/env python3
"""What lii_map_nearest costs: 100 000 queries against the 1 M-point bench map on one MI355X.

  python tools/map_nearest_cost.py [--queries 100000] [--reps 5] [--out profiles/map_nearest.md]

One process, one GPU run:
  * lii_map_nearest_dev for k in {1, 5, 16, 64} x max_dist in {1, 5}: HIP events on the handle's stream around `reps` enqueued calls
    (after two warm-up calls), and the wall clock around the same calls + lii_synchronize as a cross-check;
  * (a) k = 5, max_dist = 5 three ways, wall clock, host arrays in and out: lii_map_nearest; the route through the registration pass
    (scan_upload + downsample_skip + iekf_iterate(search) + neighbors) that was the only way to query the map before; and the k-NN
    launch of that pass alone (lii_last_timings [7]);
  * (b) oracle.Tree("ref").knn - the unmodified reference tree - with 3 threads on the same box, where oracle/_ref is built.
The queries are the points of the bench stream's scans in the world frame: what a host would ask about."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS, MAX_DISTS = (1, 5, 16, 64), (1.0, 5.0)


class Events:
    """Two HIP events on the handle's stream (the library's internal accessor: C++ linkage, not part of the C-ABI)."""

    def __init__(self, reg):
        self.hip = C.CDLL(reg.L._name)  # the runtime the library itself uses, looked up through its own handle
        get = getattr(reg.L, "_Z19lii_internal_streamP11lii_context")
        get.restype, get.argtypes = C.c_void_p, [C.c_void_p]
        self.stream = C.c_void_p(get(reg.h))
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def start(self):
        assert self.hip.hipEventRecord(self.a, self.stream) == 0

    def stop_ms(self):
        assert self.hip.hipEventRecord(self.b, self.stream) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float(0)
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return float(ms.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_nearest.md"))
    a = ap.parse_args()
    import numpy as np
    import bench
    import lidar_imu_init_amd as lii
    from oracle import oracle as O

    wl = bench.build_workload("stream100k", 2)
    world = [(s[:, :3].astype(np.float64) @ R.T + p).astype(np.float32) for s, (R, p) in zip(wl["scans"], wl["poses"])]
    q = np.ascontiguousarray(np.concatenate(world)[:a.queries])
    n, map_pts = len(q), np.ascontiguousarray(wl["map"], np.float32)
    reg = lii.Registrar(max_scan_points=n + 1024, max_map_points=int(len(map_pts) * 1.5) + 1024, filter_size_map=wl["fs_map"])
    reg.map_build(map_pts)
    ev = Events(reg)
    d_q = reg.dev_alloc(q.nbytes)
    reg._check(reg.L.lii_dev_upload(reg.h, d_q, q.ctypes.data, q.nbytes))
    d_p, d_d, d_c = reg.dev_alloc(n * 64 * 12), reg.dev_alloc(n * 64 * 4), reg.dev_alloc(n * 4)
    rows = []
    for k in KS:
        for md in MAX_DISTS:
            for _ in range(2):
                reg.map_nearest_dev(d_q, n, k, md, d_p, d_d, d_c)
            reg.synchronize()
            t0 = time.perf_counter()
            ev.start()
            for _ in range(a.reps):
                reg.map_nearest_dev(d_q, n, k, md, d_p, d_d, d_c)
            ms = ev.stop_ms() / a.reps
            reg.synchronize()
            wall = (time.perf_counter() - t0) / a.reps * 1e3
            cnt = reg.map_nearest(q[:20_000], k=k, max_dist=md)[2]
            rows.append(dict(k=k, md=md, ms=ms, wall=wall, mean_count=float(cnt.mean()), full=float((cnt == k).mean())))
            print(rows[-1], flush=True)

    def wall_of(fn, reps=3):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        return (time.perf_counter() - t0) / reps * 1e3, out

    ms_host, (hp, hd, hc) = wall_of(lambda: reg.map_nearest(q, k=5, max_dist=5.0))
    scan4 = np.ascontiguousarray(np.c_[q, np.zeros(n, np.float32)])
    ident = lii.State()

    def old_route():
        reg.scan_upload(scan4)
        m = reg.downsample_skip()
        reg.iekf_iterate(ident, True, False)
        return reg.neighbors(m)

    ms_old, (nb, nc, _) = wall_of(old_route)
    reg.set_profiling(1)
    reg.iekf_iterate(ident, True, False)
    knn_ms = reg.timings()[7]
    reg.set_profiling(0)
    same = bool(np.array_equal(nc, hc) and np.array_equal(nb[nc == 5], hp[hc == 5]))
    ref = None
    if O.ref_available():
        tree = O.Tree("ref")
        tree.build(map_pts)
        ref = {}
        for k in KS:
            for md in MAX_DISTS:
                t0 = time.perf_counter()
                tp, td, tc = tree.knn(q, k=k, max_dist=md, threads=3)
                ref[(k, md)] = (time.perf_counter() - t0) * 1e3
                print("ref", k, md, ref[(k, md)], flush=True)
        tp, td, tc = tree.knn(q, k=5, max_dist=5.0, threads=3)
        same_ref = bool(np.array_equal(tc, hc) and np.array_equal(np.where(np.isfinite(td), td, 0), hd))
    reg.close()

    lines = ["# What lii_map_nearest costs (one MI355X)", "",
             f"`python tools/map_nearest_cost.py --queries {a.queries} --reps {a.reps}`: {n} queries (points of the stream100k bench scans in the world frame) against the "
             f"{len(map_pts)}-point bench map, cell {3 * wl['fs_map']:.2f} m.  One run.", "",
             "lii_map_nearest_dev, queries and results on the device: HIP events on the handle's stream around the enqueued calls (wall clock around calls + "
             "lii_synchronize beside it)" + (", and the unmodified reference tree (`oracle.Tree(\"ref\").knn`, 3 threads, same box)." if ref else "; oracle/_ref is not built on this box: no reference tree."), "",
             "| k | max_dist | ms per call (events) | ms (wall) | ns per query | mean count | full lists | reference tree, 3 threads [ms] | tree / device |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        t = ref.get((r["k"], r["md"])) if ref else None
        lines.append(f"| {r['k']} | {r['md']:g} | {r['ms']:.3f} | {r['wall']:.3f} | {1e6 * r['ms'] / n:.1f} | {r['mean_count']:.2f} | {100 * r['full']:.1f} % | "
                     + (f"{t:.0f} | {t / r['ms']:.0f}x |" if t else "- | - |"))
    lines += ["", "k = 5, max_dist = 5, host arrays in and out (wall clock, mean of 3 calls after one):", "",
              "| route | ms |", "|---|---|",
              f"| lii_map_nearest (upload, launch, download; leaves the handle's scan alone) | {ms_host:.2f} |",
              f"| scan_upload + downsample_skip + iekf_iterate(search) + neighbors (overwrites scan, neighbour lists, have_search) | {ms_old:.2f} |",
              f"| the specialised k-NN launch of that pass alone (lii_last_timings [7]) | {knn_ms:.3f} |",
              f"| lii_map_nearest_dev, k = 5, max_dist = 5 (events, from the table) | {[r for r in rows if r['k'] == 5 and r['md'] == 5.0][0]['ms']:.3f} |", "",
              f"Both routes return the same neighbours for the full lists: {same}." + (f"  The reference tree's counts and d2 equal lii_map_nearest's: {same_ref}." if ref else ""), ""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
