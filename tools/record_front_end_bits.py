"""Records tests/golden/front_end_bits/cases.npz: the results of the cases of tests/test_gpu_front_end_bits.py with the library that is
loaded (LII_LIB names another build, e.g. the parent commit's from tools/ab_build.sh).  Needs the GPU.  Data only: every distinct
array once (blob<k>), and the table case/field -> blob (index_names, index_blob).
usage: [LII_LIB=build_ab/<name>/libliinit_hip.so] python tools/record_front_end_bits.py [out.npz]"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_front_end_bits as T  # noqa: E402
from harness import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

O.lib()
hall = synth.Hall(size=(24.0, 18.0, 6.0), n_boxes=8, seed=7)  # the small world of tests/conftest.py
got, _, _ = T.run_cases(O, (hall, hall.surface_points(0.15, noise=0.01, seed=7)))
flat = T.flatten(got)
blobs, where, names, at = {}, {}, [], []
for name in sorted(flat):
    a = np.asarray(flat[name])
    a = a if a.flags.c_contiguous else a.copy()
    key = hashlib.sha256(repr((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()
    if key not in where:
        where[key] = len(blobs)
        blobs[f"blob{len(blobs)}"] = a
    names.append(name)
    at.append(where[key])
out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
os.makedirs(os.path.dirname(out), exist_ok=True)
np.savez_compressed(out, index_names=np.array(names), index_blob=np.array(at, np.int64), **blobs)
for name in sorted(got):
    c = got[name]
    print(name, "n_down", int(c["n_down"]), "iterations", int(c.get("iterations", -2)), "effect", int(c.get("effect_num", -2)), "error", int(c.get("error", 0)))
print(f"{len(got)} cases, {len(names)} arrays, {len(blobs)} distinct -> {out} ({os.path.getsize(out)} bytes)")
