"""Feature extraction (lii_ingest_set_features) without a GPU: the plain-Python restatement tests/feature_np.py against the reference's own
output (tests/golden/features/reference_features.npz, written by tests/golden/make_feature_fixture.py from the unmodified
src/preprocess.cpp), bit for bit; every class of give_feature occurs in the fixture; the three entry points at the boundary."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import feature_cases  # noqa: E402
import feature_np  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "features", "reference_features.npz")
NEW = ["lii_ingest_set_features", "lii_ingest_corners_download", "lii_ingest_features_get"]


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def restated():
    """feature_np over every fixture case, once."""
    return {c["name"]: (c, feature_np.features(c)) for c in feature_cases.fixture_cases()}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_cases_are_the_fixtures(fixture, restated):
    assert list(fixture["names"]) == list(restated)
    for name, (case, _) in restated.items():
        assert fixture[name + "/raw"].tobytes() == case["raw"], name
        assert tuple(fixture[name + "/fields"]) == tuple(case["fields"]), name
        assert list(fixture[name + "/meta"]) == [int(case["livox"]), case["lidar_type"], case["n"], case["n_scans"], case["pfn"], case["ppl"]]
        assert list(fixture[name + "/params"]) == [case["blind"], case["stamp"]]


def test_cases_cover_the_lengths_filters_and_types(restated):
    cases = [c for c, _ in restated.values()]
    assert {c["ppl"] for c in cases} >= {1, 5, 6, 8, 9, 10, 11, 12, 63, 64, 65, 129, 700}
    for lt in (1, 2, 3):
        assert {c["pfn"] for c in cases if c["lidar_type"] == lt} >= {1, 3, 4}, lt
    assert {(c["lidar_type"], c["n_scans"]) for c in cases} >= {(1, 6), (2, 16), (3, 16), (3, 128)}
    assert any(c["lidar_type"] == 2 and c["name"].endswith("_notime") for c in cases)
    assert any(c["lidar_type"] == 2 and not c["name"].endswith("_notime") for c in cases)


def test_restatement_equals_the_reference_bit_for_bit(fixture, restated):
    for name, (_, r) in restated.items():
        surf, corn = fixture[name + "/surf"], fixture[name + "/corn"]
        assert r["surf"].shape == surf.shape and np.array_equal(_bits(r["surf"]), _bits(surf)), name
        assert r["corn"].shape == corn.shape and np.array_equal(_bits(r["corn"]), _bits(corn)), name


def test_every_lidar_type_exercises_the_unwritten_dista_read(fixture):
    for lt in (1, 2, 3):
        assert any(bool(fixture[n + "/differs_1e300"]) for n in fixture["names"] if fixture[n + "/meta"][1] == lt), lt


def test_every_class_occurs(restated):
    total = {}
    for _, r in restated.values():
        for k, v in r["stats"].items():
            total[k] = total.get(k, 0) + v
    for k in ("poss_plane", "walk_real", "small_plane", "edge_jump", "edge_plane", "wire", "mean_emitted", "remainder_lost", "group_over_64",
              "dista_tiny"):
        assert total[k] > 0, (k, total)


def test_symbols_declared_exported_mirrored_and_null_handle_refused():
    import lidar_imu_init_amd as lii
    from lidar_imu_init_amd import api
    hdr = open(os.path.join(ROOT, "include", "liinit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(lii_[a-z0-9_]+)\s*\(", code))
    L = ctypes.CDLL(lii.library_path())
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/liinit_hip.h"
        assert hasattr(L, name), f"{name} is not exported by libliinit_hip.so"
        assert name in api.EXPORTED_SYMBOLS, f"{name} is not mirrored in api.EXPORTED_SYMBOLS"
    assert all(callable(getattr(lii.Registrar, m, None)) for m in ("ingest_set_features", "ingest_corners", "ingest_features"))
    assert int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9
    assert ctypes.sizeof(api.lii_ingest_opts) == 40 and ctypes.sizeof(api.lii_frame_info) == 24
    L = lii.load_library()
    n = ctypes.c_int32(0)
    v = [ctypes.c_int32(0) for _ in range(4)]
    assert L.lii_ingest_set_features(None, 1) == -1
    assert L.lii_ingest_corners_download(None, None, None, 0, ctypes.byref(n)) == -1
    assert L.lii_ingest_features_get(None, *[ctypes.byref(x) for x in v]) == -1
    # ... and the parameter travels: reg.ingest_set_features(p.feature_extract_en)
    from lidar_imu_init_amd.params import Params
    assert Params().feature_extract_en == 0 and Params(preprocess__feature_extract_en=True).feature_extract_en == 1


@pytest.mark.skipif(not os.path.isfile("/root/reference/src/preprocess.cpp"), reason="the reference is not on this machine")
def test_generator_reproduces_the_committed_fixture(tmp_path):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_feature_fixture
    out = str(tmp_path / "again.npz")
    make_feature_fixture.main(out)
    assert open(out, "rb").read() == open(FIXTURE, "rb").read()
