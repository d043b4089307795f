#!/usr/bin/env python3
"""What feature extraction costs (lii_ingest_set_features): the whole-message ingest (cut_frame_num = 0) of the
700-points-per-line messages of tests/feature_cases.py - AVIA 6 lines, VELO 16 lines, OUSTER 128 lines - with the order on and off.

  python tools/feature_cost.py [--reps 200] [--case avia6|velo16|ouster128] [--only on|off]

Per message: a host clock around lii_ingest_livox / lii_ingest_pcl2 (the call ends in a device synchronise), `--reps` calls per form
after 20 warm-up calls, the two forms alternating in blocks of 10; mean and minimum in microseconds, one JSON line per message.  The
order off is the parent's path and bits.  For the kernels' own times run one message and one form under
`rocprofv3 --kernel-trace --stats -- python tools/feature_cost.py --case ... --only on`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"avia6": (1, 6), "velo16": (2, 16), "ouster128": (3, 128)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--case", choices=sorted(CASES), default=None)
    ap.add_argument("--only", choices=["on", "off"], default=None)
    a = ap.parse_args()
    import feature_cases
    import lidar_imu_init_amd as lii
    for key in ([a.case] if a.case else list(CASES)):
        lt, lines = CASES[key]
        c = feature_cases.bench_case(lt, lines)
        reg = lii.Registrar(max_scan_points=c["n"] + 1024, max_map_points=1000, filter_size_map=0.2)

        def one():
            if c["livox"]:
                return reg.ingest_livox(c["raw"], c["n"], c["fields"], c["n_scans"], c["pfn"], c["blind"], c["stamp"], 0, 100)
            return reg.ingest_pcl2(c["raw"], c["n"], c["fields"], c["lidar_type"], c["n_scans"], c["pfn"], c["blind"], c["stamp"], 0, 100)

        forms = [a.only] if a.only else ["off", "on"]
        times = {f: [] for f in forms}
        counts = {}
        for f in forms:
            reg.ingest_set_features(f == "on")
            for _ in range(20):
                info = one()
            counts[f] = info[0][2] if info else 0
        done = 0
        while done < a.reps:
            for f in forms:
                reg.ingest_set_features(f == "on")
                for _ in range(10):
                    t0 = time.perf_counter()
                    one()
                    times[f].append((time.perf_counter() - t0) * 1e6)
            done += 10
        feat = reg.ingest_features()
        out = dict(case=key, raw_points=c["n"], lines=lines, reps=a.reps, frame_points=counts, features=feat)
        for f in forms:
            t = sorted(times[f])
            out[f + "_us_mean"] = round(sum(t) / len(t), 1)
            out[f + "_us_min"] = round(t[0], 1)
            out[f + "_us_median"] = round(t[len(t) // 2], 1)
        print(json.dumps(out), flush=True)
        reg.close()


if __name__ == "__main__":
    main()
