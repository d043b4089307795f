"""The moving local-map cube in numpy: lasermap_fov_segment (src/laserMapping.cpp:260-305) followed by the box delete upstream prepared
and never made, restated with the widths the reference computes in - MOV_THRESHOLD = 1.5f, DET_RANGE a float32, cube_len a float64,
LocalMap_Points six float32 - so that libliinit_hip's lii_local_map_* can be held to it bit for bit.  Nothing here is timed.

    cube = LocalMapCube(cube_len=40.0, det_range=10.0)
    boxes = cube.segment(pos_end)          # (k, 6) float32, k = 0 .. 3: what Delete_Point_Boxes would get
    pts = delete_boxes(pts, boxes)         # min <= p < max on every axis
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
MOV_THRESHOLD = F32(1.5)


def constants(cube_len: float, det_range: float):
    """(thr, mov_dist): MOV_THRESHOLD * DET_RANGE in float32, and
    float(max((cube_len - 2.0 * MOV_THRESHOLD * DET_RANGE) * 0.5 * 0.9, double(DET_RANGE * (MOV_THRESHOLD - 1))))."""
    det = F32(det_range)
    thr = F32(MOV_THRESHOLD * det)
    a = (np.float64(cube_len) - np.float64(2.0) * np.float64(MOV_THRESHOLD) * np.float64(det)) * 0.5 * 0.9
    b = np.float64(F32(det * F32(MOV_THRESHOLD - F32(1))))
    return thr, F32(max(a, b))


class LocalMapCube:
    def __init__(self, cube_len: float, det_range: float):
        self.cube_len = np.float64(cube_len)
        self.thr, self.mov_dist = constants(cube_len, det_range)
        self.initialized = False
        self.vmin = np.zeros(3, F32)
        self.vmax = np.zeros(3, F32)
        self.moves = 0

    @property
    def cube(self):
        return np.concatenate([self.vmin, self.vmax]).astype(F32)

    def segment(self, pos_end) -> np.ndarray:
        """One call with state.pos_end = pos_end (the IMU's position, as upstream).  Returns cub_needrm as (k, 6) float32."""
        pos = np.asarray(pos_end, np.float64).reshape(3)
        none = np.zeros((0, 6), F32)
        if not self.initialized:
            self.vmin = (pos - self.cube_len / 2.0).astype(F32)
            self.vmax = (pos + self.cube_len / 2.0).astype(F32)
            self.initialized = True
            return none
        d0 = np.abs(pos - self.vmin.astype(np.float64)).astype(F32)
        d1 = np.abs(pos - self.vmax.astype(np.float64)).astype(F32)
        if not (np.any(d0 <= self.thr) or np.any(d1 <= self.thr)):
            return none
        old_min, old_max = self.vmin.copy(), self.vmax.copy()
        new_min, new_max = old_min.copy(), old_max.copy()
        boxes = []
        for i in range(3):  # x, y, z; the low side first, the high side by `else if`
            bmin, bmax = old_min.copy(), old_max.copy()
            if d0[i] <= self.thr:
                new_max[i] = F32(new_max[i] - self.mov_dist)
                new_min[i] = F32(new_min[i] - self.mov_dist)
                bmin[i] = F32(old_max[i] - self.mov_dist)
            elif d1[i] <= self.thr:
                new_max[i] = F32(new_max[i] + self.mov_dist)
                new_min[i] = F32(new_min[i] + self.mov_dist)
                bmax[i] = F32(old_min[i] + self.mov_dist)
            else:
                continue
            boxes.append(np.concatenate([bmin, bmax]))
        self.vmin, self.vmax = new_min, new_max
        self.moves += 1
        return np.array(boxes, F32).reshape(-1, 6)


def in_boxes(pts, boxes6) -> np.ndarray:
    """Mask of the points some box removes: min <= p < max on every axis (float32 compares, KD_TREE::Delete_by_range)."""
    p = np.asarray(pts, F32).reshape(-1, 3)
    dead = np.zeros(len(p), bool)
    for b in np.asarray(boxes6, F32).reshape(-1, 6):
        dead |= np.all((p >= b[:3]) & (p < b[3:]), axis=1)
    return dead


def delete_boxes(pts, boxes6) -> np.ndarray:
    p = np.asarray(pts, F32).reshape(-1, 3)
    return p[~in_boxes(p, boxes6)]
