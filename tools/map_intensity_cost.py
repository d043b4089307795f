"""What lii_map_intensity_set(h, 1) costs a scan's map update: two handles on the same 70 k-point hall map receive the same eight vlp16
scans in turn (de-skew + voxel filter + registration, intensities attached on both), one with the switch off and one with it on; the host
clock runs around lii_map_incremental (with counts: the call waits for the list sizes) followed by lii_synchronize.  One JSON line: the
median and the mean of the microseconds per update of either handle, and the points inserted.  usage (GPU box): python tools/map_intensity_cost.py [repeats]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import lidar_imu_init_amd as lii  # noqa: E402
from harness import synth  # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    hall = synth.Hall(size=(24.0, 18.0, 6.0), n_boxes=8, seed=7)
    map_pts = np.unique(hall.surface_points(0.15, noise=0.01, seed=7).astype(np.float32), axis=0)
    scans = []
    for k in range(8):
        R, p = synth.rot_zyx(0.03, -0.02, 0.4 + 0.05 * k), np.array([0.8 + 0.1 * k, -0.6, 0.1])
        s = synth.make_scan(hall, "vlp16", R, p, noise=0.02, seed=31 + k)
        scans.append((np.ascontiguousarray(s[np.argsort(s[:, 3], kind="stable")], np.float32), R, p))
    regs = {}
    for name in ("off", "on"):
        r = lii.Registrar(max_scan_points=40_000, max_map_points=400_000, filter_size_map=0.15)
        r.map_intensity_set(name == "on")
        r.map_build(map_pts)
        regs[name] = r
    us = {"off": [], "on": []}
    inserted = {"off": 0, "on": 0}
    for rep in range(repeats):
        for scan, R, p in scans:
            inten = np.linspace(1.0, 255.0, len(scan)).astype(np.float32)
            for name in (("off", "on") if rep % 2 == 0 else ("on", "off")):
                r = regs[name]
                st = lii.State()
                st.rot_end[:] = R
                st.pos_end[:] = p
                prop = st.copy()
                r.scan_upload(scan)
                r.scan_intensity_upload(inten)
                r.scan_register(st, prop, imu_poses=bench.pose_table(prop.rot_end, prop.pos_end), leaf=0.1, max_iterations=5, imu_en=True, scan_sorted=True)
                r.synchronize()
                t0 = time.perf_counter()
                na, nn = r.map_incremental(st)
                r.synchronize()
                us[name].append(1e6 * (time.perf_counter() - t0))
                inserted[name] += na + nn
    out = {"updates_per_handle": len(us["off"]), "points_into_the_lists": inserted}
    for name in ("off", "on"):
        a = np.array(us[name][len(scans):])  # (the first round warms the handles up)
        out[name] = {"median_us": float(np.median(a)), "mean_us": float(a.mean())}
    w = regs["on"].map_download_xyzi()[:, 3]
    out["map_points_with_intensity_on"] = int((w != 0).sum())
    out["map_points_with_intensity_off"] = int((regs["off"].map_download_xyzi()[:, 3] != 0).sum())
    print(json.dumps(out))
    for r in regs.values():
        r.close()


if __name__ == "__main__":
    main()
