"""Records tests/golden/solve_bits/cases.npz: the results of the cases of tests/test_gpu_solve_bits.py with the library that is
loaded (LII_LIB names another build, e.g. the parent commit's from tools/ab_build.sh).  Needs the GPU.
usage: [LII_LIB=build_ab/<name>/libliinit_hip.so] python tools/record_solve_bits.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_solve_bits as T  # noqa: E402
from harness import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

O.lib()
hall = synth.Hall(size=(24.0, 18.0, 6.0), n_boxes=8, seed=7)  # the small world of tests/conftest.py
got = T.run_cases(O, (hall, hall.surface_points(0.15, noise=0.01, seed=7)))
flat = {f"{name}/{f}": np.asarray(case[f]) for name, case in got.items() for f in T.FIELDS}
out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
os.makedirs(os.path.dirname(out), exist_ok=True)
np.savez_compressed(out, **flat)
for name, case in got.items():
    print(name, int(case["iterations"]), int(case["searches"]), int(case["effect_num"]), int(case["last_solve_info"]))
print(f"{len(got)} cases -> {out} ({os.path.getsize(out)} bytes)")
