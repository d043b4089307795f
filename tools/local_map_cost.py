#!/usr/bin/env python3
"""What the moving local map costs on one MI355X, on the stream100k bench stream and its map.

  python tools/local_map_cost.py [--scans 200] [--blocks 3] [--trace-stats FILE] [--out profiles/local_map.md]
  python tools/local_map_cost.py --moves-only        # the calls alone, for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...)

One process.  For a 100 000-point and the 1 000 000-point map:
  * per scan, wall clock of a Python loop of lii_scan_register calls (resident scans, IMU de-skew, voxel filter, iterated update; the
    loop's own overhead is the same on both sides): the feature off and on - a 4 000 m cube, so that nothing ever moves - in alternating
    blocks of `scans` scans; the medians of the blocks and the difference;
  * the device time of one call that does not move the cube: HIP events on the handle's stream around N_IDLE (200) enqueued
    lii_local_map_segment(out = NULL) calls - the same three launches the in-job form makes;
  * the device time of one call that moves a 40 m cube by 5 m (events around the one call: the whole delete), and what it deleted.
--trace-stats: the kernel statistics (csv) of a traced --moves-only run; the three kernels' rows are copied into the report (the tombstone
kernel alone: its largest duration is the moving call's, its smallest a call that found no box)."""
import argparse
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("k_local_map_tomb", "k_cell_apply_listed", "k_local_map_finish")
N_WARM, N_IDLE, MOVES_X = 20, 200, (5.0, 10.0, 15.0)  # calls per map that move nothing (+ the two that place a cube), and the moving ones


def kernel_rows(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("Kernel_Name") or ""
            hit = [k for k in KERNELS if k in name]
            if hit:
                rows.append((hit[0], int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
    return sorted(rows, key=lambda t: KERNELS.index(t[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--moves-only", action="store_true")
    ap.add_argument("--trace-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_map.md"))
    a = ap.parse_args()
    import numpy as np
    import bench
    import lidar_imu_init_amd as lii
    from map_nearest_cost import Events

    wl = bench.build_workload("stream100k", 8)
    full = np.ascontiguousarray(wl["map"], np.float32)
    rng = np.random.default_rng(1)
    maps = {"1M": full} if a.moves_only else {"100k": np.ascontiguousarray(full[rng.choice(len(full), 100_000, replace=False)]), "1M": full}
    results = {}
    for tag, map_pts in maps.items():
        reg = lii.Registrar(max_scan_points=max(len(s) for s in wl["scans"]) + 1024, max_map_points=int(len(map_pts) * 1.5) + 1024, filter_size_map=wl["fs_map"])
        reg.map_build(map_pts)
        ev = Events(reg)
        res = dict(points=len(map_pts))
        if not a.moves_only:
            devs = [reg.device_scan(s) for s in wl["scans"]]
            tables = [bench.pose_table(R, p) for R, p in wl["poses"]]
            states = []
            for R, p in wl["poses"]:
                st = lii.State()
                st.rot_end[:] = R
                st.pos_end[:] = p
                states.append(st)

            def block(n):
                t = np.zeros(n)
                for i in range(n):
                    k = i % len(devs)
                    st = states[k].copy()
                    t0 = time.perf_counter()
                    reg.scan_register(st, states[k], imu_poses=tables[k], leaf=wl["fs_surf"], max_iterations=wl["max_it"], imu_en=True, scan_dev=devs[k], scan_sorted=True)
                    t[i] = time.perf_counter() - t0
                return float(np.median(t) * 1e6)

            block(60)
            off, on = [], []
            for _ in range(a.blocks):
                off.append(block(a.scans))
                reg.local_map_set(4000.0, 10.0, enabled=True)
                block(20)
                on.append(block(a.scans))
                reg.local_map_set(4000.0, 10.0, enabled=False)
                block(20)
            res.update(off=off, on=on)
        # the three launches alone, nothing moves
        reg.local_map_set(4000.0, 10.0, enabled=False)
        reg.local_map_segment([0.0, 0.0, 0.0])
        for _ in range(N_WARM):
            reg.local_map_segment([0.1, 0.0, 0.0], report=False)
        reg.synchronize()
        ev.start()
        for _ in range(N_IDLE):
            reg.local_map_segment([0.1, 0.0, 0.0], report=False)
        res["idle_us"] = ev.stop_ms() / N_IDLE * 1e3
        # one real move of the 40 m cube: the slab [-20, -15) x [-20, 20) x [-20, 20) goes
        reg.local_map_set(40.0, 10.0, enabled=False)
        reg.local_map_segment([0.0, 0.0, 0.0])
        moves = []
        for x in MOVES_X:
            reg.synchronize()
            ev.start()
            reg.local_map_segment([x, 0.0, 0.0], report=False)
            ms = ev.stop_ms()
            info = reg.local_map_get()
            moves.append((ms * 1e3, info["n_deleted"]))
        res["moves"] = moves
        res["left"] = reg.map_size()
        results[tag] = res
        print(tag, res, flush=True)
        reg.close()
    if a.moves_only:
        return
    lines = ["# What the moving local map costs (one MI355X)", "",
             f"`python tools/local_map_cost.py --scans {a.scans} --blocks {a.blocks}`: the stream100k bench stream (8 resident scans of ~100 000 points) registered against "
             "its map and against a 100 000-point sample of it.  One run.", "",
             "Per scan, wall clock of a Python loop of `lii_scan_register` calls, median of each block; off = no `lii_local_map_set`, on = `enabled = 1` with a 4 000 m cube "
             "(nothing ever moves: three launches that find no box):", "",
             "| map | off, blocks [us] | on, blocks [us] | on - off, medians [us] | launches added per scan |", "|---|---|---|---|---|"]
    for tag, r in results.items():
        d = float(np.median(r["on"]) - np.median(r["off"]))
        lines.append(f"| {tag} ({r['points']} points) | {', '.join('%.1f' % v for v in r['off'])} | {', '.join('%.1f' % v for v in r['on'])} | {d:+.1f} | 3 |")
    lines += ["", "The calls alone, HIP events on the handle's stream:", "",
              f"| map | one call that moves nothing (mean of {N_IDLE} enqueued) [us] | a call that moves the 40 m cube by 5 m: whole delete [us] (points deleted) |", "|---|---|---|"]
    for tag, r in results.items():
        lines.append(f"| {tag} | {r['idle_us']:.1f} | " + "; ".join(f"{us:.0f} ({n})" for us, n in r["moves"]) + " |")
    if a.trace_stats and os.path.exists(a.trace_stats):
        lines += ["", f"Kernel durations of a traced `--moves-only` run on the 1M map ({N_WARM + N_IDLE + 2} calls that move nothing, {len(MOVES_X)} that move; the largest is a moving call's):", "",
                  "| kernel | calls | mean [us] | smallest [us] | largest [us] |", "|---|---|---|---|---|"]
        for name, calls, avg, lo, hi in kernel_rows(a.trace_stats):
            lines.append(f"| `{name}` | {calls} | {avg:.1f} | {lo:.1f} | {hi:.1f} |")
    lines.append("")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
