"""A 100 000-point ring-major scan against the bench map, registered three ways: scan_sorted = 0, = 2, and pre-sorted with = 1.
Prints the per-call host time of each form (call to return; the call ends with the result's arrival) and, given a second argument,
writes the figures to that file as JSON.  Run it plain for host times and, in a run of its own, under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/scan_sort_profile.py traced` for kernel times
(profiles/scan_sort.md).  usage (GPU box): python tools/scan_sort_profile.py [tag [out.json]]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lidar_imu_init_amd as lii  # noqa: E402
from harness import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

WARM, CALLS = int(os.environ.get("SS_WARM", 30)), int(os.environ.get("SS_CALLS", 300))
tag = sys.argv[1] if len(sys.argv) > 1 else "plain"
hall, map_pts = synth.bench_world(1_000_000, 0.15)
R, p = synth.rot_zyx(0.0, 0.01, 0.3), np.array([1.0, 2.0, 0.3])
scan = synth.make_scan(hall, "stream100k", R, p, noise=0.02, seed=5)  # ring-major: 100 rings x 1000 columns, one stamp per column
srt = O.sort_by_time(scan)
st = O.state_init()
v = O.StateView(st)
v.rot_end[:] = R
v.pos_end[:] = p
s0 = lii.State(O.state_boxplus(st, np.r_[0.002, -0.001, 0.002, 0.01, -0.01, 0.005, np.zeros(18)]))
T = lii.pose6d_array(6)
for k in range(6):
    T[k, 0] = 0.02 * k
    T[k, 4:7] = [1e-3, -2e-3, 1e-3]
    T[k, 7:10] = [1e-2, 0, 0]
    T[k, 10:13] = s0.pos_end
    T[k, 13:22] = s0.rot_end.reshape(-1)
reg = lii.Registrar(max_scan_points=120_000, max_map_points=1_300_000, filter_size_map=0.15)
reg.map_build(map_pts)
dev_u, dev_s = reg.device_scan(scan), reg.device_scan(srt)
out = dict(tag=tag, n_scan=len(scan), n_map=len(map_pts), calls=CALLS, forms={})
for name, dev, ss in (("scan_sorted=0", dev_u, 0), ("scan_sorted=2", dev_u, 2), ("presorted scan_sorted=1", dev_s, 1)):
    ts = []
    for i in range(WARM + CALLS):
        s = s0.copy()
        t0 = time.perf_counter()
        rep = reg.scan_register(s, s0, imu_poses=T, leaf=0.05, max_iterations=5, imu_en=True, scan_dev=dev, scan_sorted=ss)
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts[WARM:]) * 1e6
    out["forms"][name] = dict(host_us_median=float(np.median(ts)), host_us_mean=float(ts.mean()), host_us_p10=float(np.percentile(ts, 10)),
                              host_us_p90=float(np.percentile(ts, 90)), iterations=rep["iterations"], effect_num=rep["effect_num"],
                              pos=[float(x) for x in s.pos_end])
    print(name, out["forms"][name], flush=True)
reg.close()
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
