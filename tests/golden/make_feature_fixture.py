#!/usr/bin/env python3
"""Writes tests/golden/features/reference_features.npz: the driver messages of tests/feature_cases.py (raw bytes) together with what the
REFERENCE's own Preprocess::process returns for them with feature extraction enabled - pl_surf and pl_corn.

The reference is the unmodified src/preprocess.cpp, compiled where it lies together with tests/golden/ref_feature_wrap.cpp against
oracle/ref_shim_pre (the flags of oracle/Makefile's reference builds) into oracle/_ref/libref_feature.so; this script only runs where
the reference exists.  Two of its reads touch memory nobody wrote (disB, types[plsize - 1].dista); the wrapper holds both at 0 - the
library's definition - and every case is run a second time with dista preset to 1e300 to record whether that read decided anything.

Conditions asserted here (not measurements): at least one case per lidar type differs under the 1e300 preset; no kept point of any case
has range < blind, no line is blind throughout and no OUSTER line is empty (the reference's undefined spots stay out of the fixture)."""
import ctypes as C
import io
import os
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import feature_cases  # noqa: E402
import feature_np  # noqa: E402
from harness import wire  # noqa: E402

REF = os.environ.get("LII_REFERENCE", "/root/reference")
LIB = os.path.join(ROOT, "oracle", "_ref", "libref_feature.so")
OUT = os.path.join(HERE, "features", "reference_features.npz")


def build_lib():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-O3", "-std=c++14", "-fopenmp", "-fPIC", "-shared", "-w",
           "-I" + os.path.join(ROOT, "oracle", "ref_shim_pre"), "-I" + os.path.join(REF, "src"),
           os.path.join(HERE, "ref_feature_wrap.cpp"), os.path.join(REF, "src", "preprocess.cpp"), "-o", LIB]
    subprocess.run(cmd, check=True)
    return C.CDLL(LIB)


def run_ref(lib, case, preset):
    raw = np.frombuffer(case["raw"], np.uint8)
    cap = case["n"] + 16
    surf = np.zeros((cap, 4), np.float32)
    corn = np.zeros((cap, 5), np.float32)
    nc = C.c_int(0)
    fields = (C.c_int * len(case["fields"]))(*case["fields"])
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    if case["livox"]:
        lib.ref_features_livox.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_void_p]
        ns = lib.ref_features_livox(p(raw), case["n"], fields, case["n_scans"], case["pfn"], case["blind"], preset, p(surf), p(corn), cap,
                                    C.byref(nc))
    else:
        lib.ref_features_pcl2.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_void_p]
        ns = lib.ref_features_pcl2(p(raw), case["n"], fields, case["lidar_type"], case["n_scans"], case["pfn"], case["blind"], preset, p(surf),
                                   p(corn), cap, C.byref(nc))
    assert ns >= 0, (case["name"], ns)
    return surf[:ns].copy(), corn[:nc.value].copy()


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def save_npz(path, arrays):
    """np.savez_compressed with fixed member times: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main(out_path=OUT):
    assert os.path.isfile(os.path.join(REF, "src", "preprocess.cpp")), "the reference is not here"
    lib = build_lib()
    out = {}
    names = []
    differs_by_type = {}
    for case in feature_cases.fixture_cases():
        # the reference's undefined spots stay out of the fixture
        for l, (xyz, _, _) in enumerate(feature_np.collect(case)):
            L = feature_np._Line(xyz, case["lidar_type"], case["blind"])
            assert not (L.range < case["blind"]).any(), (case["name"], l, "a kept point with range < blind")
            assert case["lidar_type"] != wire.OUSTER or L.n > 0, (case["name"], l, "an empty OUSTER line")
        surf, corn = run_ref(lib, case, 0.0)
        surf2, corn2 = run_ref(lib, case, 0.0)
        assert same(surf, surf2) and same(corn, corn2), (case["name"], "two runs with the same preset differ")
        surf_big, corn_big = run_ref(lib, case, 1e300)
        differs = not (same(surf, surf_big) and same(corn, corn_big))
        differs_by_type[case["lidar_type"]] = differs_by_type.get(case["lidar_type"], False) or differs
        c = case["name"]
        names.append(c)
        out[c + "/raw"] = np.frombuffer(case["raw"], np.uint8)
        out[c + "/fields"] = np.array(case["fields"], np.int32)
        # livox, lidar_type, n, n_scans, point_filter_num, points per line
        out[c + "/meta"] = np.array([int(case["livox"]), case["lidar_type"], case["n"], case["n_scans"], case["pfn"], case["ppl"]], np.int32)
        out[c + "/params"] = np.array([case["blind"], case["stamp"]])
        out[c + "/surf"] = surf
        out[c + "/corn"] = corn
        out[c + "/differs_1e300"] = np.array(differs)
        print(f"{c}: {len(surf)} surf, {len(corn)} corn, differs under 1e300: {differs}")
    for lt in (wire.AVIA, wire.VELO, wire.OUSTER):
        assert differs_by_type.get(lt), f"no case of lidar type {lt} differs under the 1e300 preset"
    out["names"] = np.array(names)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    save_npz(out_path, out)
    size = os.path.getsize(out_path)
    print("wrote", out_path, size, "bytes")
    assert size < 800_000, size


if __name__ == "__main__":
    main(*sys.argv[1:2])
