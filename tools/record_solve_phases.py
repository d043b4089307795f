"""Records tests/golden/solve_phases/cases.npz: the results of the cases of tests/test_gpu_solve_phases.py (the fused launch) with
the library that is loaded (LII_LIB names another build, e.g. the parent commit's from tools/ab_build.sh), and says whether the
three-launch form and the host-driven sums of that library agree with them.  Needs the GPU.
usage: [LII_LIB=build_ab/<name>/libliinit_hip.so] python tools/record_solve_phases.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_solve_phases as T  # noqa: E402
from harness import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

O.lib()
hall = synth.Hall(size=(24.0, 18.0, 6.0), n_boxes=8, seed=7)  # the small world of tests/conftest.py
got = T.run_cases(O, (hall, hall.surface_points(0.15, noise=0.01, seed=7)))
flat = {f"{name}/{f}": np.asarray(case[f]) for name, case in got["fused"].items() for f in T.FIELDS}
out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
os.makedirs(os.path.dirname(out), exist_ok=True)
np.savez_compressed(out, **flat)
for name, case in got["fused"].items():
    three = all(np.array_equal(case[f], got["three"][name][f]) for f in T.FIELDS)
    dth = np.linalg.norm(O.log_so3(case["start"][0:9].reshape(3, 3).T @ case["state"][0:9].reshape(3, 3)))
    print(f"{name:18s} it {int(case['iterations'])} searches {int(case['searches'])} effect {int(case['effect_num'])} converged {int(case['converged'])} "
          f"solve_info {int(case['last_solve_info'])} |dtheta| {dth:.2e}  three-launch form: {'same bits' if three else 'DIFFERS'}")
for name, s in got["sums91"].items():
    print(f"{name}: k_reduce91 alone {'same bits as' if np.array_equal(s, got['fused'][name]['normal_eq']) else 'DIFFERS from'} the fused launch's sums")
print(f"{len(got['fused'])} cases -> {out} ({os.path.getsize(out)} bytes)")
