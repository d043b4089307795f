"""CPU-side checks of the time sort's boundary: lii_scan_sort is declared, exported and mirrored, the ABI number and the job's
fields are what they were (scan_sorted = 2 is a new VALUE of an existing field), and the Python arguments map onto it."""
import ctypes
import os
import re

import pytest

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "liinit_hip.h")).read()


def test_scan_sort_is_declared_exported_and_mirrored():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"\bint\s+lii_scan_sort\s*\(\s*lii_handle\s+h\s*\)\s*;", code)
    L = ctypes.CDLL(lii.library_path())
    assert hasattr(L, "lii_scan_sort")
    assert "lii_scan_sort" in api.EXPORTED_SYMBOLS
    assert callable(getattr(lii.Registrar, "scan_sort"))
    # a null handle is refused without touching a device
    assert lii.load_library().lii_scan_sort(None) == -1  # LII_ERR_INVALID


def test_abi_number_and_job_fields_are_unchanged():
    assert int(re.search(r"#define\s+LII_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 9
    assert lii.load_library().lii_abi_version() == 9
    body = HEADER[HEADER.index("typedef struct lii_scan_job {"):HEADER.index("} lii_scan_job;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"^\s*(?:const\s+)?[A-Za-z_0-9]+\*?\s+\*?\(?\*?([a-z_0-9]+)\)?(?:\(void\* arg\))?;", body, re.M)
    assert fields == ["struct_size", "undistort", "imu_poses", "n_imu_poses", "leaf", "opts", "scan_dev", "n_scan_dev", "scan_sorted",
                      "map_update", "next_scan_dev", "next_n_scan", "reserved1", "while_waiting", "while_waiting_arg"], fields
    assert [f[0] for f in api.lii_scan_job._fields_] == fields
    assert ctypes.sizeof(api.lii_scan_job) == 88 and api.lii_scan_job.scan_sorted.offset == 44


def test_header_describes_the_new_value():
    body = HEADER[HEADER.index("typedef struct lii_scan_job {"):HEADER.index("} lii_scan_job;")]
    assert "2: sort this scan by time on the device first" in body
    assert "scan_sorted = 2" in HEADER[HEADER.index("ORDER OF THE POINTS"):HEADER.index("lii_undistort_imu <-")]
    assert "with scan_sorted = 2" in HEADER[HEADER.index("cut_frame_num = 0"):HEADER.index("`data` is sensor_msgs")]


@pytest.mark.parametrize("arg,value", [(False, 0), (0, 0), (True, 1), (1, 1), (2, 2), ("sort", 2)])
def test_python_scan_sorted_argument(arg, value):
    assert api.scan_sorted_value(arg) == value


def test_python_scan_sorted_argument_refuses_other_words():
    with pytest.raises(ValueError):
        api.scan_sorted_value("sorted")
