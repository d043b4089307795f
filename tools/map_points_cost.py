#!/usr/bin/env python3
"""What the map edits and queries by point and box cost on the 1 M-point bench map (one MI355X): profiles/map_points.md.

  python tools/map_points_cost.py [--reps 5] [--json out.json] [--parent parent.json] [--out profiles/map_points.md]

Wall clock around the synchronous calls (each returns with its result on the host), two warm-up calls, then `reps` calls: median and
minimum.  Every repeat deletes OTHER stored points (a delete changes the map; under a tenth of the 1 M points go over the whole run).
On a checkout that has no lii_map_delete_points - the parent commit - only the routes that exist there are timed
(lii_map_delete_boxes with one-ulp boxes, lii_map_download + host min / max / box filter): copy this file into a checkout of it; its
--json goes into this commit's run as --parent, and the table sets the two side by side."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import bench
    import lidar_imu_init_amd as lii

    wl = bench.build_workload("stream100k", 2)
    map_pts = np.ascontiguousarray(wl["map"], np.float32)
    reg = lii.Registrar(max_scan_points=120_000, max_map_points=int(len(map_pts) * 1.5) + 1024, filter_size_map=wl["fs_map"])
    reg.map_build(map_pts)
    new = hasattr(reg, "map_delete_points")
    rng = np.random.default_rng(1)
    stored = reg.map_download()
    stored = stored[(stored != 0).all(axis=1)]
    stored = np.ascontiguousarray(stored[rng.permutation(len(stored))])
    cursor = [0]

    def take(n):
        p = stored[cursor[0]:cursor[0] + n]
        cursor[0] += n
        assert len(p) == n
        return p

    def ulp_boxes(p):
        return np.concatenate([p, np.nextafter(p, np.float32(np.inf))], axis=1).astype(np.float32)

    def timed(fn, make_arg, check=None):
        ts = []
        for r in range(a.reps + 2):
            arg = make_arg()
            t0 = time.perf_counter()
            out = fn(arg)
            dt = (time.perf_counter() - t0) * 1e3
            if check is not None:
                check(arg, out)
            if r >= 2:
                ts.append(dt)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "reps": a.reps}

    res = {"map_points": int(len(map_pts)), "new": new}
    centre = map_pts[len(map_pts) // 2]  # (a box around a stored point: the middle of the hall is empty)
    box = np.concatenate([centre - np.float32(2.0), centre + np.float32(2.0)]).astype(np.float32)[None]

    def n_equals(n):
        def check(arg, out):
            assert out == n, (out, n)
        return check

    for n in (256, 4096):
        res[f"delete_boxes_ulp_{n}"] = timed(reg.map_delete_boxes, lambda: ulp_boxes(take(n)), n_equals(n))
        print(n, "boxes", res[f"delete_boxes_ulp_{n}"], flush=True)
        if new:
            res[f"delete_points_{n}"] = timed(reg.map_delete_points, lambda: take(n), n_equals(n))
            print(n, "points", res[f"delete_points_{n}"], flush=True)
            d = reg.dev_alloc(n * 12)

            def dev(p):
                reg.dev_upload(d, p)
                t0 = time.perf_counter()
                reg.map_delete_points_dev(d, n)
                reg.synchronize()
                return (time.perf_counter() - t0) * 1e3

            for _ in range(2):
                dev(take(n))
            ts = [dev(take(n)) for _ in range(a.reps)]
            res[f"delete_points_dev_{n}"] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "reps": a.reps}
            print(n, "points, dev", res[f"delete_points_dev_{n}"], flush=True)

    def host_range(_):
        p = reg.map_download()
        return np.concatenate([p.min(axis=0), p.max(axis=0)])

    def host_box(_):
        p = reg.map_download()
        return p[((box[0, :3] <= p) & (p < box[0, 3:])).all(axis=1)]

    res["download_minmax"] = timed(host_range, lambda: None)
    res["download_box_filter"] = timed(host_box, lambda: None)
    want_r, want_b = host_range(None), host_box(None)
    res["box_hits"] = int(len(want_b))
    if new:
        res["map_range"] = timed(lambda _: reg.map_range(), lambda: None)
        res["map_box_search"] = timed(lambda _: reg.map_box_search(box), lambda: None)
        assert np.array_equal(reg.map_range().view(np.uint32), want_r.astype(np.float32).view(np.uint32))
        got = reg.map_box_search(box)
        key = lambda x: x[np.lexsort((x[:, 2], x[:, 1], x[:, 0]))]
        assert np.array_equal(key(got), key(want_b))
    reg.close()
    print(json.dumps(res, indent=1), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)
    if not (a.out and new):
        return
    par = json.load(open(a.parent)) if a.parent else None

    def cell(d, k):
        return f"{d[k]['median_ms']:.3f} ({d[k]['min_ms']:.3f})" if d and k in d else "-"

    L = ["# What the map edits and queries by point and box cost (one MI355X)", "",
         f"`python tools/map_points_cost.py --reps {a.reps}` on this commit" + (f" (on top of {a.commit})" if a.commit else "") +
         (", and the same script on the parent commit, which times the routes that exist there" if par else "") +
         f": the {len(map_pts)}-point stream100k bench map, cell {3 * wl['fs_map']:.2f} m.  Wall clock around the synchronous calls, ms, "
         f"median (minimum) of {a.reps} calls after two; every repeat deletes other stored points.  One run each.", "",
         "| call | this commit | parent commit |", "|---|---|---|"]
    for n in (256, 4096):
        L.append(f"| lii_map_delete_points, {n} stored points (host list in, count out) | {cell(res, f'delete_points_{n}')} | - |")
        L.append(f"| lii_map_delete_points_dev, {n} points + lii_synchronize | {cell(res, f'delete_points_dev_{n}')} | - |")
        L.append(f"| lii_map_delete_boxes, the {n} one-ulp boxes [p, nextafter p) | {cell(res, f'delete_boxes_ulp_{n}')} | {cell(par, f'delete_boxes_ulp_{n}')} |")
    L += [f"| lii_map_range | {cell(res, 'map_range')} | - |",
          f"| lii_map_download + host min / max | {cell(res, 'download_minmax')} | {cell(par, 'download_minmax')} |",
          f"| lii_map_box_search, one 4 m box ({res['box_hits']} points) | {cell(res, 'map_box_search')} | - |",
          f"| lii_map_download + host box filter | {cell(res, 'download_box_filter')} | {cell(par, 'download_box_filter')} |", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    main()
