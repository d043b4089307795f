"""Driver messages for the feature-extraction path (preprocess/feature_extract_en; lii_ingest_set_features), test data only.

Scene: rays cast from the sensor onto an axis-aligned room of 10 m half-width with a box face at x = 6 m (depth jumps, corners), a 2 cm
pole 3 m away (one ray per line hits it: Wire), the +y side open (no return beyond inf_bound: the records are zero and fall to the blind
test) and one pair of consecutive identical points per line (the dista < 1e-16 branches).  The messages are packed in the layouts of
harness/wire.py.  `fixture_cases()` are the ones the reference pins (tests/golden/make_feature_fixture.py); `extra_cases()` touch what
the reference leaves undefined (kept points with range < blind, a line blind throughout, an empty OUSTER line) and are held to
tests/feature_np.py alone."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from harness import wire  # noqa: E402

AZ_STEP_DEG = 0.5
AZ0_DEG = -30.0
POLE_COL = 500  # (columns beyond a line's length simply have no pole)
POLE_R = 3.0


def _cast(az, el):
    """Range along each ray (nan: no return)."""
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = 10.0 / np.abs(d[:, 0])
        ty = 10.0 / np.abs(d[:, 1])
        tz = np.where(d[:, 2] < 0, 3.0 / np.abs(d[:, 2]), 3.5 / np.abs(d[:, 2]))
        t = np.minimum(np.minimum(tx, ty), tz)
        open_side = (ty <= tx) & (ty <= tz) & (d[:, 1] > 0)
        tb = 6.0 / d[:, 0]  # the box face x = 6, |y| <= 2
        hit_box = (d[:, 0] > 0) & (np.abs(tb * d[:, 1]) <= 2.0) & (tb < t)
    t = np.where(hit_box, tb, t)
    t = np.where(open_side & ~hit_box, np.nan, t)
    return d, t


def _lines(n_lines, ppl, seed, fov_deg=15.0):
    """xyz (n_lines, ppl, 3) float32, time offset [ms] (n_lines, ppl)."""
    rng = np.random.default_rng(seed)
    col = np.arange(ppl)
    az = np.deg2rad(AZ0_DEG + AZ_STEP_DEG * col)
    xyz = np.zeros((n_lines, ppl, 3), np.float32)
    for l in range(n_lines):
        el = np.deg2rad(-fov_deg + 2 * fov_deg * (l + 0.5) / n_lines)
        d, t = _cast(az, np.full(ppl, el))
        t = t + rng.normal(0, 0.002, ppl)
        if POLE_COL < ppl:
            t[POLE_COL] = POLE_R / np.cos(el)
        p = np.where(np.isfinite(t)[:, None], d * np.where(np.isfinite(t), t, 0.0)[:, None], 0.0).astype(np.float32)
        if ppl >= 6:  # the identical pair, at a place that moves with the line
            k = 2 + (l * 7) % (ppl - 3)
            p[k + 1] = p[k]
        xyz[l] = p
    t_ms = np.broadcast_to(col * (100.0 / max(ppl, 1)), (n_lines, ppl)).copy()
    return xyz, t_ms


def _pcl2(lidar_type, n_lines, ppl, seed, with_time=True, stray=True):
    xyz, t_ms = _lines(n_lines, ppl, seed, 15.0 if n_lines <= 16 else 22.0)
    # firing order: all rings of column 0, then column 1, ...
    xyz = xyz.transpose(1, 0, 2).reshape(-1, 3)
    t = t_ms.T.reshape(-1) + np.tile(np.arange(n_lines) * 1e-3, ppl)
    ring = np.tile(np.arange(n_lines), ppl).astype(np.int32)
    if stray and len(ring) > 40:  # records of rings the sensor does not have (ring >= N_SCANS): extra records, the lines keep their length
        rng = np.random.default_rng(seed + 1)
        at = np.sort(rng.choice(len(ring), 5, replace=False))
        xyz = np.insert(xyz, at, xyz[at], axis=0)
        t = np.insert(t, at, t[at])
        ring = np.insert(ring, at, n_lines + 4)
    a = np.zeros(len(xyz), wire.DTYPES[lidar_type])
    a["x"], a["y"], a["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    a["ring"] = ring
    a["intensity"] = (np.arange(len(xyz)) % 97).astype(np.float32)
    if lidar_type == wire.VELO:
        a["time"] = (t / 1000.0).astype(np.float32) if with_time else 0.0
    else:
        a["t"] = np.round(t * 1e6).astype(np.uint32)
    return a.tobytes(), len(a)


def _livox(n_lines, ppl, seed):
    xyz, t_ms = _lines(n_lines, ppl, seed)
    xyz = xyz.transpose(1, 0, 2).reshape(-1, 3)
    t = t_ms.T.reshape(-1) + np.tile(np.arange(n_lines) * 1e-3, ppl)
    line = np.tile(np.arange(n_lines), ppl).astype(np.uint8)
    tag = np.full(len(line), 0x10, np.uint8)
    # one leading record (the reference's loop starts at 1) and, when the message is long enough, a few strays
    xyz = np.insert(xyz, 0, [[5.0, 0.0, 0.0]], axis=0)
    t = np.insert(t, 0, 0.0)
    line = np.insert(line, 0, 0)
    tag = np.insert(tag, 0, 0x10)
    if len(line) > 40:
        rng = np.random.default_rng(seed + 1)
        at = np.sort(rng.choice(np.arange(2, len(line)), 6, replace=False))
        xyz = np.insert(xyz, at, xyz[at] + np.float32(0.5), axis=0)
        t = np.insert(t, at, t[at])
        line = np.insert(line, at, [n_lines + 1, n_lines + 1, 0, 1, n_lines + 1, 2])
        tag = np.insert(tag, at, [0x00, 0x10, 0x20, 0x30, 0x00, 0x20])  # (tag 0x00 at a line >= N_SCANS passes the test and is dropped)
        tag[np.arange(len(tag)) % 11 == 3] &= 0xCF  # tag 0x00 on lines the sensor has: kept
        tag |= (np.arange(len(tag)) % 16).astype(np.uint8)  # low bits are unrelated flags
    a = np.zeros(len(xyz), wire.LIVOX_DTYPE)
    a["x"], a["y"], a["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    a["offset_time"] = np.round(t * 1e6).astype(np.uint32)
    a["reflectivity"] = np.arange(len(xyz)) % 251
    a["line"] = line
    a["tag"] = tag
    return a.tobytes(), len(a)


def _case(name, lidar_type, n_scans, ppl, pfn, raw, n, blind=1.0, stamp=100.25):
    livox = lidar_type == wire.AVIA
    return dict(name=name, livox=livox, lidar_type=lidar_type, n_scans=n_scans, ppl=ppl, pfn=pfn, blind=blind, stamp=stamp, raw=raw, n=n,
                fields=wire.livox_fields() if livox else wire.pc2_fields(lidar_type))


# (lidar, lines, points per line, point_filter_num, per-point time): every length of the issue's list once, every type at every filter
_FIXTURE = [
    (wire.AVIA, 6, 700, 3, True), (wire.VELO, 16, 65, 1, True), (wire.OUSTER, 16, 129, 4, True),
    (wire.VELO, 16, 129, 3, False), (wire.OUSTER, 128, 65, 1, True), (wire.OUSTER, 16, 64, 3, True), (wire.VELO, 16, 63, 3, True), (wire.VELO, 16, 64, 4, True),
    (wire.AVIA, 6, 129, 1, True), (wire.AVIA, 6, 12, 4, True), (wire.VELO, 16, 11, 4, True), (wire.OUSTER, 16, 10, 1, True),
    (wire.AVIA, 6, 9, 1, True), (wire.VELO, 16, 8, 3, False), (wire.AVIA, 6, 6, 1, True), (wire.AVIA, 6, 5, 1, True),
    (wire.VELO, 16, 1, 1, True), (wire.OUSTER, 16, 5, 1, True), (wire.VELO, 16, 2, 1, False), (wire.OUSTER, 16, 1, 1, True),
]
_NAMES = {wire.AVIA: "avia", wire.VELO: "velo", wire.OUSTER: "ouster"}


def _build(lt, lines, ppl, pfn, with_time, seed):
    if lt == wire.AVIA:
        raw, n = _livox(lines, ppl, seed)
    else:
        raw, n = _pcl2(lt, lines, ppl, seed, with_time)
    return _case(f"{_NAMES[lt]}_{lines}x{ppl}_pfn{pfn}{'' if with_time else '_notime'}", lt, lines, ppl, pfn, raw, n)


def fixture_cases():
    return [_build(lt, lines, ppl, pfn, wt, 40 + k) for k, (lt, lines, ppl, pfn, wt) in enumerate(_FIXTURE)]


def _rewrite(case, fn):
    livox = case["livox"]
    a = np.frombuffer(case["raw"], wire.LIVOX_DTYPE if livox else wire.DTYPES[case["lidar_type"]]).copy()
    fn(a, a["line"] if livox else a["ring"])
    out = dict(case)
    out["raw"] = a.tobytes()
    return out


def extra_cases():
    """What the reference leaves undefined; the library's definitions (include/liinit_hip.h) are restated in tests/feature_np.py."""
    out = []
    for lt, lines, ppl, pfn in [(wire.VELO, 16, 129, 3), (wire.OUSTER, 16, 65, 1), (wire.AVIA, 6, 129, 1)]:
        base = _build(lt, lines, ppl, pfn, True, 90 + lt)

        def near_axis(a, line, lt=lt):  # kept (3-D range >= blind) with a horizontal range below it: every 9th record
            m = np.arange(len(a)) % 9 == 4
            a["x"][m], a["y"][m], a["z"][m] = 0.05, 0.02, 2.0 + 0.01 * (np.arange(m.sum()) % 7)
        c = _rewrite(base, near_axis)
        c["name"] = base["name"] + "_range_below_blind"
        out.append(c)

        def blind_line(a, line):  # line 2 blind throughout
            m = line == 2
            a["x"][m], a["y"][m] = 0.05, 0.02
            a["z"][m] = 2.0 + 0.01 * np.arange(m.sum())
        c = _rewrite(base, blind_line)
        c["name"] = base["name"] + "_blind_line"
        out.append(c)
    base = _build(wire.OUSTER, 16, 65, 3, True, 97)

    def empty_line(a, ring):
        ring[ring == 3] = 40
    c = _rewrite(base, empty_line)
    c["name"] = base["name"] + "_empty_line"
    out.append(c)
    return out


def bench_case(lidar_type, lines, ppl=700, pfn=1):
    """The messages the measurement of profiles/features.md times."""
    return _build(lidar_type, lines, ppl, pfn, True, 7)
