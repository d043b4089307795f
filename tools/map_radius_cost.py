#!/usr/bin/env python3
"""What lii_map_radius_dev costs: the 2 000 queries of the suite's small_world set against its 68 k-point hall
map on one MI355X, max_dist in {1, 5, 30}.

  python tools/map_radius_cost.py [--reps 20] [--out profiles/map_radius.md]

One process, one GPU run.  HIP events on the handle's stream (tools/map_nearest_cost.Events) around `reps` enqueued calls after two
warm-up calls, per max_dist:
  * A: offsets and total only (pts_dev = d2_dev = NULL): the count pass + the scan + the copy of the total;
  * S: the same call for queries that are all NaN - no query walks a cell: an empty count launch + the scan + the copy, the
    upper bound of what the scan costs; A - S is the count pass;
  * B: the full unsorted call; B - A is the fill pass;
  * C: the full call with LII_RADIUS_SORTED; C - B is the sorted extra (key fill instead of row fill, radix sort, gather);
  * the yardstick: lii_map_nearest_dev with k = 64 on the same queries, in the same run.
Bytes written per call are computed from the shapes: 8 (n + 1) + 8 of offsets and total, 16 per row."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MAX_DISTS = (1.0, 5.0, 30.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_radius.md"))
    a = ap.parse_args()
    import numpy as np
    import lidar_imu_init_amd as lii
    from harness import synth
    from map_nearest_cases import query_set
    from map_nearest_cost import Events

    hall = synth.Hall(size=(24.0, 18.0, 6.0), n_boxes=8, seed=7)  # tests/conftest.py: small_world
    map_pts = np.ascontiguousarray(hall.surface_points(0.15, noise=0.01, seed=7), np.float32)
    q = np.ascontiguousarray(query_set(hall, map_pts))
    n = len(q)
    reg = lii.Registrar(max_scan_points=10_000, max_map_points=100_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    ev = Events(reg)
    d_q, d_nan = reg.dev_alloc(q.nbytes), reg.dev_alloc(q.nbytes)
    reg.dev_upload(d_q, q)
    reg.dev_upload(d_nan, np.full_like(q, np.nan))
    d_o, d_t = reg.dev_alloc(8 * (n + 1)), reg.dev_alloc(8)
    d_c = reg.dev_alloc(4 * n)

    def timed(call):
        for _ in range(2):
            call()
        reg.synchronize()
        ev.start()
        for _ in range(a.reps):
            call()
        return ev.stop_ms() / a.reps

    rows = []
    for md in MAX_DISTS:
        total = int(reg.map_radius(q, md, points=False)[0][-1])
        d_p, d_d = reg.dev_alloc(12 * total), reg.dev_alloc(4 * total)
        r = dict(md=md, total=total,
                 A=timed(lambda: reg.map_radius_dev(d_q, n, md, d_o, None, None, 0, d_t)),
                 S=timed(lambda: reg.map_radius_dev(d_nan, n, md, d_o, None, None, 0, d_t)),
                 B=timed(lambda: reg.map_radius_dev(d_q, n, md, d_o, d_p, d_d, total, d_t)),
                 C=timed(lambda: reg.map_radius_dev(d_q, n, md, d_o, d_p, d_d, total, d_t, sorted=True)))
        d_np, d_nd = reg.dev_alloc(n * 64 * 12), reg.dev_alloc(n * 64 * 4)
        r["knn64"] = timed(lambda: reg.map_nearest_dev(d_q, n, 64, md, d_np, d_nd, d_c))
        rows.append(r)
        print(r, flush=True)
    reg.close()

    lines = ["# What lii_map_radius costs (one MI355X)", "",
             f"`python tools/map_radius_cost.py --reps {a.reps}`: the {n} queries of the suite's small_world set against its {len(map_pts)}-point hall map, cell 0.45 m.  "
             "One run; HIP events on the handle's stream around the enqueued calls of lii_map_radius_dev, queries and results on the device.", "",
             "count pass = (offsets-only call) - (the same call for NaN queries, which walk nothing); scan = that NaN call: an empty count launch + the exclusive scan "
             "+ the copy of the total (an upper bound of the scan); fill pass = (full call) - (offsets-only call); sorted extra = (LII_RADIUS_SORTED call) - (full call).  "
             "The yardstick is lii_map_nearest_dev with k = 64 on the same queries in the same run.  Bytes written: 8 (n + 1) + 8 of offsets and total, 16 a row.", "",
             "| max_dist | rows | count pass [ms] | scan [ms] | fill pass [ms] | full call [ms] | sorted extra [ms] | sorted call [ms] | lii_map_nearest_dev k = 64 [ms] | bytes written | ns per row (full call) |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        written = 8 * (n + 1) + 8 + 16 * r["total"]
        lines.append(f"| {r['md']:g} | {r['total']} | {r['A'] - r['S']:.3f} | {r['S']:.3f} | {r['B'] - r['A']:.3f} | {r['B']:.3f} | {r['C'] - r['B']:.3f} | {r['C']:.3f} | "
                     f"{r['knn64']:.3f} | {written} | {1e6 * r['B'] / max(r['total'], 1):.2f} |")
    lines.append("")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
