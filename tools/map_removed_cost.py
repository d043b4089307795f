#!/usr/bin/env python3
"""What the history of removed points (lii_map_removed_set) costs the moving local map, on the 1 M-point map of
profiles/local_map.md.  One process, one library build (LII_LIB selects another one - the parent commit's from tools/ab_build.sh, which
lacks the order: its `on` figures are left out); run it alternating between the builds and compare the JSON lines.

  python tools/map_removed_cost.py [--rounds 3]

Per round, HIP events on the handle's stream (tools/map_nearest_cost.Events), order off and - where the library has it - on:
  * one call that moves nothing: the mean over 200 enqueued lii_local_map_segment(out = NULL) calls of a 4 000 m cube;
  * one call that moves a 40 m cube by 5 m, three moves after a fresh map_build: the whole delete, and the points each move removed
    (and, with the order on, held / lost afterwards).
Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_WARM, N_IDLE, MOVES_X = 20, 200, (5.0, 10.0, 15.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import bench
    import lidar_imu_init_amd as lii
    from map_nearest_cost import Events

    wl = bench.build_workload("stream100k", 8)
    map_pts = np.ascontiguousarray(wl["map"], np.float32)
    reg = lii.Registrar(max_scan_points=4096, max_map_points=int(len(map_pts) * 1.5) + 1024, filter_size_map=wl["fs_map"])
    has_order = hasattr(reg.L, "lii_map_removed_set")
    ev = Events(reg)
    out = dict(library=os.environ.get("LII_LIB", "tree"), points=len(map_pts), idle_off_us=[], idle_on_us=[], move_off=[], move_on=[])

    def idle():
        reg.local_map_set(4000.0, 10.0, enabled=False)
        reg.local_map_segment([0.0, 0.0, 0.0])
        for _ in range(N_WARM):
            reg.local_map_segment([0.1, 0.0, 0.0], report=False)
        reg.synchronize()
        ev.start()
        for _ in range(N_IDLE):
            reg.local_map_segment([0.1, 0.0, 0.0], report=False)
        return round(ev.stop_ms() / N_IDLE * 1e3, 2)

    def moves():
        reg.map_build(map_pts)
        reg.local_map_set(40.0, 10.0, enabled=False)
        reg.local_map_segment([0.0, 0.0, 0.0])
        got = []
        for x in MOVES_X:
            reg.synchronize()
            ev.start()
            reg.local_map_segment([x, 0.0, 0.0], report=False)
            us = ev.stop_ms() * 1e3
            got.append((round(us, 1), reg.local_map_get()["n_deleted"]))
        return got

    reg.map_build(map_pts)
    for _ in range(a.rounds):
        orders = [False, True] if has_order else [False]
        for on in orders:
            if has_order:
                reg.map_removed_set(300_000 if on else 0)
            out["idle_on_us" if on else "idle_off_us"].append(idle())
            m = moves()
            if on:
                info = reg.map_removed_get()
                assert info["held"] == sum(n for _, n in m) and info["lost_total"] == 0, info
                reg.map_removed_acquire(clear=True)
            out["move_on" if on else "move_off"].append(m)
    reg.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
