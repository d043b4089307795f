"""One scan point at a time through lii_fit.hip: the plane of its five neighbours, the two gates, its Jacobian row and what it adds to
the 91 sums, against the per-point numpy reference (tests/plane_rows_np.py) and the oracle - on every path a point can take to its fit.

lii_iekf_iterate returns the 91 sums of a scan.  With ONE point in the scan they are that point's row; with one live point among filler
points whose rows are exactly zero they are the same bits, wherever the live point sits.  The map is a set of isolated clusters, so the
five neighbours of every query are known; the query's distance to its cluster decides whether the search pass finishes it (d5 < 0.16 m^2)
or flags it for a completion path (d5 > 0.81 m^2), and lii_last_unfinished_queries says which it was.  tests/test_plane_rows_host.py
asserts all of these preconditions, the branch coverage of the QR and the exclusion cap on the CPU.

Which test reaches which path, and how that is asserted:
  k_fit_reduce<true, true>    a, c (n <= 131 072), d, e - every search pass here is host-driven, behind a search launch
  k_fit_reduce<true, false>   b, c (n <= 131 072), e - the pass on cached planes
  k_fit_reduce<false, true>   c at n = 131 073 (513 workgroups; launch_fit_reduce takes the instance by the scan's size), search pass
  k_fit_reduce<false, false>  c at n = 131 073, cached planes
  finished by the search      a: near queries, last_unfinished_queries == 0
  complete_one_coop           a: far queries, last_unfinished_queries == 1 (one flagged query: one completion workgroup, m == 1); d at u = 1, 96
  several handed through LDS  d at u = 97 and 256 (97 .. 256 flagged: some completion workgroup holds two and more), unfinished == u
  complete_flagged            d at u = 257 and e (more than kFlagCap flagged: every workgroup finishes its own), unfinished == u
  canon_ties                  a, c, e: family H - the tied points stand in the map in descending x, the downloaded list must be ascending
  the all-zero matrix          own_maps: five map points at the origin - count 5, not selected, 91 zeros, both passes, near and far query
  nzp 1 / 2 / 3, tau = 0, norm re-computation, six pivot orders: a, over families D / C / all, C and D, G, F - the host test asserts the
                              reference took each branch on these inputs, the device must produce the same plane.

Tolerances: the device's sums against each reference, per group, within 8 x the CPU discrepancy between the two references
(plane_rows_np.DISC: out[0:78] over rinv |h|^2, out[78:90] over rinv |h| |z|); lists, counts, selection flags and every "same point, other
place" comparison are exact.  Sums of many points: math.fsum of the points' single-point device rows within (n - 1) 2^-53 sum |addend|.
"""
import numpy as np
import pytest

import plane_rows_np as pr

pytestmark = pytest.mark.gpu

TOL_HH = pr.DEVICE_FACTOR * pr.DISC["hh"]
TOL_HZ = pr.DEVICE_FACTOR * pr.DISC["hz"]
PLACEMENT_CFG = ("lio", True)
F_N = 300


@pytest.fixture(scope="module")
def m(oracle):
    return pr.measure(oracle)


@pytest.fixture(scope="module")
def cs():
    return pr.cases()


def _registrar(cs, max_scan_points):
    import lidar_imu_init_amd as lii
    reg = lii.Registrar(max_scan_points=max_scan_points, max_map_points=4096, filter_size_map=0.15)
    reg.map_build(cs.map)
    assert reg.map_size() == len(cs.map)   # every point is kept, the exact duplicates of family D included
    return reg


@pytest.fixture(scope="module")
def reg(cs):
    r = _registrar(cs, 2048)
    yield r
    r.close()


@pytest.fixture(scope="module")
def reg_big(cs):
    r = _registrar(cs, 131_200)
    yield r
    r.close()


def run_scan(reg, bodies, pod, pod2, imu_en, world=False):
    """One search pass at `pod`, then one pass on cached planes at `pod2`.  Returns dict(out, nb, cnt, sel, unfinished, out2, sel2)."""
    import lidar_imu_init_amd as lii
    scan = pr.scan_of(bodies)
    reg.scan_upload(scan)
    n = reg.downsample_skip()
    assert n == len(scan)
    out = reg.iekf_iterate(lii.State(pod), True, imu_en)
    unfinished = reg.last_unfinished_queries()
    nb, cnt, sel = reg.neighbors(n)
    r = dict(out=out, nb=nb, cnt=cnt, sel=sel.astype(bool), unfinished=unfinished)
    if world:
        r["world"] = np.ascontiguousarray(reg.scan_download(2)[:, :3])
    r["out2"] = reg.iekf_iterate(lii.State(pod2), False, imu_en)
    _, _, sel2 = reg.neighbors(n)
    r["sel2"] = sel2.astype(bool)
    return r


_single = {}


@pytest.fixture(scope="module")
def single(reg, m):
    """single(key): the one-point scans of every query of a CONFIGS entry on the device, run once."""
    def get(key):
        if key not in _single:
            c = m["cfg"][key]
            _single[key] = [run_scan(reg, b[None, :], c["pod"], c["pod2"], key[1]) for b in c["body"]]
        return _single[key]
    yield get
    _single.clear()


def _check_point(tag, r, o, f, cnt, nb, sel, out, worst):
    """One point's list, count, selection flag and - where `out` is its own row - sums against both references."""
    assert cnt == r["count"], (tag, cnt, r["count"])
    assert np.array_equal(nb[:cnt].view(np.uint32), r["nb"][:cnt].view(np.uint32)), (tag, nb, r["nb"])
    if pr.excluded(r, f):
        worst["left out"] += 1
        return
    assert bool(sel) == r["selected"], (tag, sel, r["selected"], r["margin"])
    assert bool(sel) == o["selected"], (tag, "oracle")
    if "nb" in o:
        assert cnt == o["count"] and np.array_equal(nb[:cnt].view(np.uint32), o["nb"][:cnt].view(np.uint32)), (tag, "oracle")
    if out is None:
        return
    assert out[90] == float(r["selected"]), (tag, out[90])
    if not r["selected"]:
        assert not np.any(out), (tag, out)
        return
    for name, ref_out in (("numpy", None), ("oracle", o["out"])):
        a, b = pr.group_ratios(out, r, TOL_HH, TOL_HZ, f, ref_out=ref_out)
        worst[name + " hh"], worst[name + " hz"] = max(worst[name + " hh"], a), max(worst[name + " hz"], b)
        assert a <= 1.0 and b <= 1.0, (tag, name, a, b, "x the tolerance (out[0:78], out[78:90])", r["margin"])


def _worst():
    return {"numpy hh": 0.0, "numpy hz": 0.0, "oracle hh": 0.0, "oracle hz": 0.0, "left out": 0}


def _report(label, worst):
    print(f"\n[{label}] worst device difference / tolerance (8 x CPU discrepancy): "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items() if k != "left out") + f"; left out {worst['left out']}")


# ------------------------------------------------------------------------------------------------ a, b
@pytest.mark.parametrize("key", pr.CONFIGS, ids=lambda k: f"{k[0]}-imu{int(k[1])}")
def test_single_point_search_pass(cs, m, single, key):
    c = m["cfg"][key]
    dev = single(key)
    worst = _worst()
    kinds = {"F": 0, "U": 0}
    for k, (r, o, f, d) in enumerate(zip(c["ref"], c["orc"], c["fam"], dev)):
        q = cs.queries[c["ids"][k]]
        tag = (key, int(c["ids"][k]), f, cs.nh[q["nh"]]["tag"], q["kind"], q["tag"])
        _check_point(tag, r, o, f, int(d["cnt"][0]), d["nb"][0], d["sel"][0], d["out"], worst)
        if c["F"][k]:
            assert d["unfinished"] == 0, tag    # finished by the search pass
            kinds["F"] += 1
        if c["U"][k]:
            assert d["unfinished"] == 1, tag    # flagged: the one query of one completion workgroup
            kinds["U"] += 1
    _report(f"a {key}", worst)
    assert kinds["F"] >= F_N and kinds["U"] >= 257
    assert worst["left out"] <= pr.EXCLUDE_CAP * len(dev)


@pytest.mark.parametrize("key", pr.CONFIGS, ids=lambda k: f"{k[0]}-imu{int(k[1])}")
def test_single_point_cached_plane(cs, m, single, key):
    """The pass on cached planes at the moved pose: the row at the new pose with the plane of the first pass; a point is a candidate only
    if the first pass selected it (tests/test_plane_rows_host.py: the moved pose deselects some, and some the first pass left out would
    pass now - they must stay out)."""
    c = m["cfg"][key]
    dev = single(key)
    worst = _worst()
    for k, (r1, r, o, f, d) in enumerate(zip(c["ref"], c["ref2"], c["orc2"], c["fam"], dev)):
        tag = (key, int(c["ids"][k]), f, "cached")
        if pr.excluded(r1, f) or pr.excluded(r, f):
            worst["left out"] += 1
            continue
        if not r1["selected"]:
            assert not d["sel2"][0] and not np.any(d["out2"]), tag
        _check_point(tag, r, o, f, int(d["cnt"][0]), d["nb"][0], d["sel2"][0], d["out2"], worst)
    _report(f"b {key}", worst)
    assert worst["left out"] <= pr.EXCLUDE_CAP * len(dev)


@pytest.fixture(scope="module")
def reg_own():
    import lidar_imu_init_amd as lii
    r = lii.Registrar(max_scan_points=64, max_map_points=1024, filter_size_map=0.15)
    yield r
    r.close()


@pytest.mark.parametrize("key", pr.CONFIGS, ids=lambda k: f"{k[0]}-imu{int(k[1])}")
def test_single_point_own_maps(m, reg_own, key):
    """The neighbourhoods that need a map of their own (plane_rows_np.MiniMaps), one-point scans, search pass and cached planes: generic
    patches 0.5 - 4 m from the origin, and the all-zero matrix - five map points AT the origin: every column norm 0, 0 / 0 in the solve, a
    NaN plane that passes the plane test and a NaN s that fails the gate - count 5, not selected, 91 zeros in both passes, for a query the
    search finishes and one it flags, under every pose."""
    mm = pr.minimaps()
    c = m["mini"][key]
    worst, worst2 = _worst(), _worst()
    zeros = 0
    current = None
    for k, qi in enumerate(c["ids"]):
        nh = mm.queries[qi]["nh"]
        if nh != current:
            reg_own.map_build(mm.nh[nh]["pts"])
            assert reg_own.map_size() == len(mm.nh[nh]["pts"])
            current = nh
        d = run_scan(reg_own, c["body"][k][None, :], c["pod"], c["pod2"], key[1])
        r, r2, f = c["ref"][k], c["ref2"][k], c["fam"][k]
        tag = (key, int(qi), f, mm.nh[nh]["tag"], mm.queries[qi]["kind"])
        _check_point(tag, r, c["orc"][k], f, int(d["cnt"][0]), d["nb"][0], d["sel"][0], d["out"], worst)
        if not (pr.excluded(r, f) or pr.excluded(r2, f)):
            _check_point(tag + ("cached",), r2, c["orc2"][k], f, int(d["cnt"][0]), d["nb"][0], d["sel2"][0], d["out2"], worst2)
        assert d["unfinished"] == (0 if c["F"][k] else 1), tag
        assert c["F"][k] or c["U"][k], tag
        if f == "Z":
            assert d["cnt"][0] == 5 and not np.any(d["nb"][0]) and not d["sel"][0] and not d["sel2"][0], tag
            assert not np.any(d["out"]) and not np.any(d["out2"]), tag
            zeros += 1
    _report(f"own maps, search pass {key}", worst)
    _report(f"own maps, cached planes {key}", worst2)
    assert zeros == 2 and worst["left out"] + worst2["left out"] <= pr.EXCLUDE_CAP * 2 * len(c["ids"])


# ------------------------------------------------------------------------------------------------ c
def _live_cases(cs, c):
    """About a dozen live points: generic near and far, ties, rank 2 and rank 1, both sides of both gates, the match bound."""
    want = [("A", "near", None), ("A", "far", None), ("F", "near", None), ("F", "far", None), ("H", "near", None), ("H", "far", None),
            ("C", "near", "line"), ("D", "near", "close"), ("B", "near", "inside"), ("B", "near", "outside"), ("J", "near", "gate 0.99"),
            ("J", "near", "gate 1.01"), ("I", "far", "d5 = 5"), ("G", "far", None)]
    picked = []
    for fam, kind, tag in want:
        for k, qi in enumerate(c["ids"]):
            q = cs.queries[qi]
            nh = cs.nh[q["nh"]]
            if nh["family"] == fam and q["kind"] == kind and (tag is None or tag in nh["tag"] or tag == q["tag"]) and k not in picked:
                if fam in "AFHCG" and not c["ref"][k]["selected"]:
                    continue
                picked.append(k)
                break
        else:
            raise AssertionError((fam, kind, tag))
    return picked


@pytest.mark.parametrize("n", [2, 5, 255, 256, 257, 1025, 131_072, 131_073])
def test_placement_among_filler(cs, m, single, reg_big, n):
    """One live point at index i of an n-point scan of filler: the sums are the bits of the live point's one-point scan, in the search
    pass and on cached planes; its list and flag are its own, nobody else is selected.  n = 131 073 is the smallest scan that launches
    k_fit_reduce<false, .> (more than 512 workgroups)."""
    key = PLACEMENT_CFG
    c = m["cfg"][key]
    dev = single(key)
    live = _live_cases(cs, c)
    assert sum(c["ref"][k]["selected"] for k in live) >= 8 and sum(not c["ref"][k]["selected"] for k in live) >= 2
    filler = cs.filler_bodies(key[0], n)
    places = sorted({0, 3, 4, n - 1, n - 2, 4 * ((n - 1) // 4)} & set(range(n)))
    for k in live:
        one = dev[k]
        for i in places:
            bodies = filler.copy()
            bodies[i] = c["body"][k]
            d = run_scan(reg_big, bodies, c["pod"], c["pod2"], key[1])
            tag = (n, i, int(c["ids"][k]), c["fam"][k])
            assert np.array_equal(d["out"], one["out"]), (tag, "search pass", d["out"] - one["out"])
            assert np.array_equal(d["out2"], one["out2"]), (tag, "cached planes", d["out2"] - one["out2"])
            assert d["unfinished"] == one["unfinished"], tag
            assert d["cnt"][i] == one["cnt"][0] and np.array_equal(d["nb"][i].view(np.uint32), one["nb"][0].view(np.uint32)), tag
            assert d["sel"][i] == one["sel"][0] and d["sel2"][i] == one["sel2"][0], tag
            assert d["sel"].sum() == int(one["sel"][0]) and d["sel2"].sum() == int(one["sel2"][0]), tag
            others = np.arange(n) != i
            assert np.all(d["cnt"][others] == 5), tag


# ------------------------------------------------------------------------------------------------ d, e
def _check_scan(label, cs, c, dev, picks, d, worst, key):
    """A scan of the queries `picks` (indices into the configuration's queries): per-point lists, counts and flags against the reference,
    the sums against math.fsum of the points' one-point device rows."""
    rows, rows2 = [], []
    for at, k in enumerate(picks):
        r, f = c["ref"][k], c["fam"][k]
        tag = (label, at, int(c["ids"][k]), f)
        _check_point(tag, r, c["orc"][k], f, int(d["cnt"][at]), d["nb"][at], d["sel"][at], None, worst)
        # the same point in its one-point scan: the same flag, exactly (no exclusion: the same arithmetic on the same inputs)
        assert d["sel"][at] == dev[k]["sel"][0] and d["sel2"][at] == dev[k]["sel2"][0], tag
        rows.append(dev[k]["out"])
        rows2.append(dev[k]["out2"])
    for name, out, rr in (("search pass", d["out"], rows), ("cached planes", d["out2"], rows2)):
        total, bound = pr.fsum_rows(rr)
        assert out[90] == total[90], (label, name)
        assert np.all(np.abs(out - total) <= bound), (label, name, np.max(np.abs(out - total) / np.maximum(bound, 1e-300)))


@pytest.mark.parametrize("u", [1, 96, 97, 256, 257])
def test_completion_paths(cs, m, single, reg, u):
    """F_N queries the search pass finishes and u it flags: 1 .. 96 go one per completion workgroup (complete_one_coop), 97 .. 256 leave
    workgroups with several, handed to their fitting lanes through LDS, more than 256 are finished by every workgroup for itself
    (complete_flagged)."""
    key = PLACEMENT_CFG
    c = m["cfg"][key]
    dev = single(key)
    near = np.flatnonzero(c["F"])[:F_N]
    far = np.flatnonzero(c["U"])
    far = far[np.arange(u) % len(far)]
    picks = np.r_[near, far]
    picks = picks[np.random.default_rng(9100 + u).permutation(len(picks))]
    d = run_scan(reg, c["body"][picks], c["pod"], c["pod2"], key[1])
    assert d["unfinished"] == u
    worst = _worst()
    _check_scan(f"d u={u}", cs, c, dev, picks, d, worst, key)
    assert d["sel"].sum() >= 200


@pytest.mark.parametrize("key", pr.CONFIGS, ids=lambda k: f"{k[0]}-imu{int(k[1])}")
def test_whole_set_at_once(cs, m, single, reg, key):
    c = m["cfg"][key]
    dev = single(key)
    picks = np.arange(len(c["ids"]))
    d = run_scan(reg, c["body"], c["pod"], c["pod2"], key[1], world=True)
    assert d["unfinished"] >= int(c["U"].sum()) > 256
    assert np.array_equal(d["world"].view(np.uint32), np.ascontiguousarray([r["world"] for r in c["ref"]]).view(np.uint32))
    worst = _worst()
    _check_scan(f"e {key}", cs, c, dev, picks, d, worst, key)
