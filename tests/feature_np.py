"""Plain-Python restatement of the feature-extraction path (reference src/preprocess.cpp: the feature branches of avia_handler :373-418,
oust_handler :487-536 and velodyne_handler :585-652, give_feature :715-965, plane_judge :976-1071, edge_jump_judge :1073-1102).
TEST-ONLY.  Every decision is an IEEE add / mul / div / sqrt in the reference's types and order.  Where the reference reads memory nobody
wrote, or runs off an array, this file states the LIBRARY's definition (include/liinit_hip.h):
  disB = 0;  types[plsize - 1].dista = 0;  a line blind throughout yields nothing;  an empty line yields nothing;  vecs[j] next to a
  blind neighbour is the zero vector (the quotient is NaN, every comparison with it false);  a plane group that runs off the end of its
  line marks the points the line has.
features(case) -> dict(surf (n, 4) f32: x y z curvature; corn (m, 5) f32: x y z intensity curvature; ftype: per line uint8 array;
                      n_lines: lines the passes ran on; stats: how often each class / event occurred)."""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from harness import wire  # noqa: E402

NOR, POSS_PLANE, REAL_PLANE, EDGE_JUMP, EDGE_PLANE, WIRE = 0, 1, 2, 3, 4, 5
NR_NOR, NR_ZERO, NR_180, NR_INF, NR_BLIND = 0, 1, 2, 3, 4

F32, F64 = np.float32, np.float64
GROUP_SIZE = 8
DIS_A, DIS_B = 0.1, 0.0  # (the constructor's second assignment; disB is never initialised: 0 here)
INF_BOUND = 10.0
P2L_RATIO = 225.0
LIMIT_MAXMID, LIMIT_MIDMIN, LIMIT_MAXMIN = 6.25, 6.25, 3.24
JUMP_UP_LIMIT = math.cos(170.0 / 180 * math.pi)
JUMP_DOWN_LIMIT = math.cos(8.0 / 180 * math.pi)
COS160 = math.cos(160.0 / 180 * math.pi)
SMALLP_INTERSECT = math.cos(172.5 / 180 * math.pi)
SMALLP_RATIO = 1.2
EDGE_A, EDGE_B = 2.0, 0.1


def thresholds():
    """(jump_up_limit, jump_down_limit, cos160, smallp_intersect): src/preprocess.cpp:30-33."""
    return JUMP_UP_LIMIT, JUMP_DOWN_LIMIT, COS160, SMALLP_INTERSECT


def _sq3(x, y, z):  # float arithmetic: x * x + y * y + z * z
    return (x * x + y * y) + z * z


def collect(case):
    """pl_buff: per line (xyz (k, 3) f32, intensity (k,) f32, curvature (k,) f32), message order kept."""
    n, N, blind = case["n"], case["n_scans"], case["blind"]
    lt = case["lidar_type"]
    empty = (np.zeros((0, 3), F32), np.zeros(0, F32), np.zeros(0, F32))
    if n == 0:
        return [empty for _ in range(N)]
    if case["livox"]:
        a = np.frombuffer(case["raw"], wire.LIVOX_DTYPE)
        x, y, z = a["x"].copy(), a["y"].copy(), a["z"].copy()
        line = a["line"].astype(np.int64)
        tag = a["tag"] & 0x30
        idx = np.arange(n)
        pop = (idx >= 1) & (((line < N) & (tag == 0x10)) | (tag == 0x00))
        fx, fy, fz = np.where(pop, x, F32(0)), np.where(pop, y, F32(0)), np.where(pop, z, F32(0))  # pl_full
        px, py, pz = np.roll(fx, 1), np.roll(fy, 1), np.roll(fz, 1)
        px[0] = py[0] = pz[0] = 0
        d = _sq3(x, y, z).astype(F64)
        differs = (np.abs(x - px).astype(F64) > 1e-7) | (np.abs(y - py).astype(F64) > 1e-7) | (np.abs(z - pz).astype(F64) > 1e-7)
        keep = pop & ~(d < blind * blind) & differs & (line < N)
        curv = a["offset_time"].astype(F32) / F32(1000000)
        inten = a["reflectivity"].astype(F32)
    else:
        a = np.frombuffer(case["raw"], wire.DTYPES[lt])
        x, y, z = a["x"].copy(), a["y"].copy(), a["z"].copy()
        line = a["ring"].astype(np.int64)
        with np.errstate(invalid="ignore"):
            d = _sq3(x, y, z).astype(F64)
            ok = ~((d < blind * blind) | np.isnan(x) | np.isnan(y) | np.isnan(z))
        keep = ok & (line < N)
        inten = a["intensity"].copy()
        if lt == wire.OUSTER:
            curv = (a["t"].astype(F64) / 1e6).astype(F32)
        else:
            curv = (a["time"].astype(F64) * 1000.0).astype(F32)
            if not (a["time"][n - 1] > 0):  # the constant-rotation model: a recurrence per ring, whose first point only seeds it
                keep = keep.copy()
                first, yaw_fp, time_last = {}, {}, {}
                omega_l = 3.61
                for i in np.nonzero(keep)[0]:
                    layer = int(line[i])
                    yaw = math.atan2(float(y[i]), float(x[i])) * 57.2957
                    if layer not in first:
                        first[layer] = True
                        yaw_fp[layer] = yaw
                        time_last[layer] = F32(0)
                        keep[i] = False
                        continue
                    if yaw <= yaw_fp[layer]:
                        c = F32((yaw_fp[layer] - yaw) / omega_l)
                    else:
                        c = F32((yaw_fp[layer] - yaw + 360.0) / omega_l)
                    if c < time_last[layer]:
                        c = F32(float(c) + 360.0 / omega_l)
                    time_last[layer] = c
                    curv[i] = c
    out = []
    for l in range(N):
        m = keep & (line == l)
        out.append((np.stack([x[m], y[m], z[m]], -1).astype(F32).reshape(-1, 3), inten[m].astype(F32), curv[m].astype(F32)))
    return out


class _Line:
    def __init__(self, xyz, lt, blind):
        self.n = len(xyz)
        self.xf, self.yf, self.zf = xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy()
        self.X, self.Y, self.Z = self.xf.astype(F64), self.yf.astype(F64), self.zf.astype(F64)
        r = self.xf * self.xf + self.yf * self.yf  # float
        self.range = (r if lt == wire.AVIA else np.sqrt(r)).astype(F64)
        vx = (self.xf[:-1] - self.xf[1:]).astype(F64)
        vy = (self.yf[:-1] - self.yf[1:]).astype(F64)
        vz = (self.zf[:-1] - self.zf[1:]).astype(F64)
        self.dista = np.concatenate([(vx * vx + vy * vy) + vz * vz, [0.0]])  # (the last one is never written: 0 here)
        self.lt, self.blind = lt, blind
        self.ftype = np.zeros(self.n, np.uint8)
        self.intersect = np.full(self.n, 2.0)


def _plane_judge(L, i_cur):
    """-> (type, i_nex, direct)"""
    n, blind = L.n, L.blind
    group_dis = DIS_A * L.range[i_cur] + DIS_B
    group_dis = group_dis * group_dis
    zero = (0.0, 0.0, 0.0)
    for j in range(i_cur, i_cur + GROUP_SIZE):
        if L.range[j] < blind:
            return 2, j, zero
    j0 = i_cur + GROUP_SIZE
    vx = (L.xf[j0:] - L.xf[i_cur]).astype(F64)
    vy = (L.yf[j0:] - L.yf[i_cur]).astype(F64)
    vz = (L.zf[j0:] - L.zf[i_cur]).astype(F64)
    two = (vx * vx + vy * vy) + vz * vz
    isblind = L.range[j0:] < blind
    stop = np.nonzero(isblind | (two >= group_dis))[0]
    if len(stop):
        k = int(stop[0])
        i_nex = j0 + k
        if isblind[k]:
            return 2, i_nex, zero
    else:
        k = n - 1 - j0  # ran off the line: vx, vy, vz, two_dis are those of the last point
        i_nex = n
    vx, vy, vz, two_dis = vx[k], vy[k], vz[k], two[k]
    hi = min(i_nex, n)
    leng_wid = F64(0.0)
    if hi > i_cur + 1:
        a0 = (L.xf[i_cur + 1:hi] - L.xf[i_cur]).astype(F64)
        a1 = (L.yf[i_cur + 1:hi] - L.yf[i_cur]).astype(F64)
        a2 = (L.zf[i_cur + 1:hi] - L.zf[i_cur]).astype(F64)
        b0 = a1 * vz - vy * a2
        b1 = a2 * vx - a0 * vz
        b2 = a0 * vy - vx * a1
        lw = (b0 * b0 + b1 * b1) + b2 * b2
        lw = lw[lw > 0.0]  # (`if (lw > leng_wid)` from 0: NaN and 0 never enter)
        if len(lw):
            leng_wid = lw.max()
    if two_dis * two_dis / leng_wid < P2L_RATIO:
        return 0, i_nex, zero
    s = np.sort(L.dista[i_cur:i_nex])[::-1]
    m = len(s)
    if s[m - 2] < 1e-16:
        return 0, i_nex, zero
    if L.lt == wire.AVIA:
        if s[0] / s[m // 2] >= LIMIT_MAXMID or s[m // 2] / s[m - 2] >= LIMIT_MIDMIN:
            return 0, i_nex, zero
    elif s[0] / s[m - 2] >= LIMIT_MAXMIN:
        return 0, i_nex, zero
    nrm = np.sqrt((vx * vx + vy * vy) + vz * vz)
    return 1, i_nex, (vx / nrm, vy / nrm, vz / nrm)


def _edge_jump_judge(L, i, nor_dir):
    blind = L.blind
    if nor_dir == 0:
        if L.range[i - 1] < blind or L.range[i - 2] < blind:
            return False
    else:
        if L.range[i + 1] < blind or L.range[i + 2] < blind:
            return False
    d1 = L.dista[i + nor_dir - 1]
    d2 = L.dista[i + 3 * nor_dir - 2]
    if d1 < d2:
        d1, d2 = d2, d1
    d1, d2 = np.sqrt(d1), np.sqrt(d2)
    return not (d1 > EDGE_A * d2 or (d1 - d2) > EDGE_B)


def _norm(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def give_feature(L, inten, curv, pfn, surf, corn, stats):
    n, blind = L.n, L.blind
    if n == 0:
        return
    below = L.range < blind
    if below.all():
        return  # (the reference's head search runs off the line)
    head = int(np.argmin(below))
    ft = L.ftype
    # 1. the plane walk
    plsize2 = n - GROUP_SIZE if n > GROUP_SIZE else 0
    last_state, last_direct = 0, (F64(0), F64(0), F64(0))
    i = head
    while i < plsize2:
        if L.range[i] < blind:
            i += 1
            continue
        ptype, i_nex, direct = _plane_judge(L, i)
        if i_nex - i > 64:
            stats["group_over_64"] += 1
        if ptype == 1:
            hi = min(i_nex, n - 1)
            ft[i:hi + 1] = REAL_PLANE
            ft[i] = POSS_PLANE
            if i_nex < n:
                ft[i_nex] = POSS_PLANE
            stats["walk_plane"] += 1
            if last_state == 1 and _norm(last_direct) > 0.1:
                mod = _dot(last_direct, direct)
                ft[i] = EDGE_PLANE if (mod > -0.707 and mod < 0.707) else REAL_PLANE
            i = i_nex - 1
            last_state = 1
        else:
            i = i_nex
            last_state = 0
        last_direct = direct
        i += 1
    stats["walk_real"] += int((ft == REAL_PLANE).sum())
    # 2. edge jumps and wires
    plsize2 = n - 3 if n > 3 else 0
    for i in range(head + 3, plsize2):
        if L.range[i] < blind or ft[i] >= REAL_PLANE:
            continue
        if L.dista[i - 1] < 1e-16 or L.dista[i] < 1e-16:
            stats["dista_tiny"] += 1
            continue
        va = (L.X[i], L.Y[i], L.Z[i])
        edj = [NR_NOR, NR_NOR]
        vecs = [(F64(0), F64(0), F64(0)), (F64(0), F64(0), F64(0))]
        for j, m in ((0, -1), (1, 1)):
            if L.range[i + m] < blind:
                edj[j] = NR_INF if L.range[i] > INF_BOUND else NR_BLIND
                continue
            v = (L.X[i + m] - va[0], L.Y[i + m] - va[1], L.Z[i + m] - va[2])
            vecs[j] = v
            angle = _dot(va, v) / _norm(va) / _norm(v)
            if angle < JUMP_UP_LIMIT:
                edj[j] = NR_180
            elif angle > JUMP_DOWN_LIMIT:
                edj[j] = NR_ZERO
        inter = _dot(vecs[0], vecs[1]) / _norm(vecs[0]) / _norm(vecs[1])
        L.intersect[i] = inter
        dp, dc = L.dista[i - 1], L.dista[i]
        if edj[0] == NR_NOR and edj[1] == NR_ZERO and dc > 0.0225 and dc > 4 * dp:
            if inter > COS160 and _edge_jump_judge(L, i, 0):
                ft[i] = EDGE_JUMP
        elif edj[0] == NR_ZERO and edj[1] == NR_NOR and dp > 0.0225 and dp > 4 * dc:
            if inter > COS160 and _edge_jump_judge(L, i, 1):
                ft[i] = EDGE_JUMP
        elif edj[0] == NR_NOR and edj[1] == NR_INF:
            if _edge_jump_judge(L, i, 0):
                ft[i] = EDGE_JUMP
        elif edj[0] == NR_INF and edj[1] == NR_NOR:
            if _edge_jump_judge(L, i, 1):
                ft[i] = EDGE_JUMP
        elif edj[0] > NR_NOR and edj[1] > NR_NOR:
            if ft[i] == NOR:
                ft[i] = WIRE
    # 3. small planes: a firing at i turns i + 1 into Real_Plane and thereby keeps it from firing
    for i in range(head + 1, n - 1):
        if L.range[i] < blind or L.range[i - 1] < blind or L.range[i + 1] < blind:
            continue
        if L.dista[i - 1] < 1e-8 or L.dista[i] < 1e-8:
            continue
        if ft[i] == NOR:
            if L.dista[i - 1] > L.dista[i]:
                ratio = L.dista[i - 1] / L.dista[i]
            else:
                ratio = L.dista[i] / L.dista[i - 1]
            if L.intersect[i] < SMALLP_INTERSECT and ratio < SMALLP_RATIO:
                if ft[i - 1] == NOR:
                    ft[i - 1] = REAL_PLANE
                if ft[i + 1] == NOR:
                    ft[i + 1] = REAL_PLANE
                ft[i] = REAL_PLANE
                stats["small_plane"] += 1
    # 4. emission
    last_surface = -1
    for j in range(head, n):
        if ft[j] == POSS_PLANE or ft[j] == REAL_PLANE:
            if last_surface == -1:
                last_surface = j
            if j == last_surface + pfn - 1:
                surf.append((L.xf[j], L.yf[j], L.zf[j], curv[j]))
                last_surface = -1
        else:
            if ft[j] == EDGE_JUMP or ft[j] == EDGE_PLANE:
                corn.append((L.xf[j], L.yf[j], L.zf[j], inten[j], curv[j]))
            if last_surface != -1:
                ap = [F32(0), F32(0), F32(0), F32(0)]
                for k in range(last_surface, j):
                    ap[0] = ap[0] + L.xf[k]
                    ap[1] = ap[1] + L.yf[k]
                    ap[2] = ap[2] + L.zf[k]
                    ap[3] = ap[3] + curv[k]
                c = F32(j - last_surface)
                surf.append((ap[0] / c, ap[1] / c, ap[2] / c, ap[3] / c))
                stats["mean_emitted"] += 1
            last_surface = -1
    if last_surface != -1:
        stats["remainder_lost"] += 1


def features(case):
    lt, pfn = case["lidar_type"], case["pfn"]
    stats = dict(walk_plane=0, walk_real=0, small_plane=0, mean_emitted=0, remainder_lost=0, group_over_64=0, dista_tiny=0)
    surf, corn, ftypes = [], [], []
    n_lines = 0
    with np.errstate(all="ignore"):
        for xyz, inten, curv in collect(case):
            L = _Line(xyz, lt, case["blind"])
            skip = (lt == wire.AVIA and L.n <= 5) or (lt == wire.VELO and L.n < 2) or L.n == 0
            if not skip:
                n_lines += 1
                give_feature(L, inten, curv, pfn, surf, corn, stats)
            ftypes.append(L.ftype)
    for name, code in (("poss_plane", POSS_PLANE), ("real_plane", REAL_PLANE), ("edge_jump", EDGE_JUMP), ("edge_plane", EDGE_PLANE), ("wire", WIRE)):
        stats[name] = int(sum(int((f == code).sum()) for f in ftypes))
    return dict(surf=np.array(surf, F32).reshape(-1, 4), corn=np.array(corn, F32).reshape(-1, 5), ftype=ftypes, n_lines=n_lines, stats=stats)
