// The moving local-map cube: lasermap_fov_segment (src/laserMapping.cpp:260-305), ONE definition of its arithmetic for the launch that
// decides inside a registration (position read from the update's control block) and for lii_local_map_segment (position by value).
// MOV_THRESHOLD = 1.5f, DET_RANGE a float, cube_len a double, LocalMap_Points six floats.  The two per-configuration constants - thr =
// 1.5f * det_range and mov_dist - are formed on the HOST when the setting is made (lii_local_map_set) and arrive here as numbers.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace lii {

// The cube and what the last call did with it.  Two of these live in device memory (a call reads one and writes the other, so every
// workgroup of the launch that decides sees the same cube), one in pinned host memory (the report).
struct LocalMapState {
  float cube[6];        // LocalMap_Points: min xyz, max xyz
  int initialized;      // Localmap_Initialized
  int n_boxes;          // cub_needrm of the last call
  float boxes[18];
  int moves;            // calls that moved the cube
  int n_deleted;        // points the last call's boxes removed
  int n_valid;          // live points of the map behind the last call
  int seq;              // number of the last call.  Not a hand-over word: the pinned copy is written with one plain store of the whole
                        // struct and is read by the host only behind a later launch of the same stream (the update's result, a synchronise)
  long long deleted_total;
};
struct LocalMapParams {
  double cube_len;
  float thr;       // MOV_THRESHOLD * DET_RANGE
  float mov_dist;
};

// dist_to_map_edge of the three axes (low face, high face) and need_move: is any of the six within the threshold?
__host__ __device__ inline bool fov_need_move(const float cube[6], const double pos[3], float thr, float d0[3], float d1[3]) {
  bool need_move = false;
  for (int i = 0; i < 3; i++) {
    d0[i] = (float)fabs(pos[i] - (double)cube[i]);
    d1[i] = (float)fabs(pos[i] - (double)cube[3 + i]);
    if (d0[i] <= thr || d1[i] <= thr) need_move = true;
  }
  return need_move;
}

// One lasermap_fov_segment() at pos (= state.pos_end: the IMU's position, as upstream).  `out` = the cube afterwards, the boxes to
// delete (none on the initialising call and when nothing moved) and moves + 1 when the cube moved.
__host__ __device__ inline void fov_segment_dev(const LocalMapState& in, const double pos[3], const LocalMapParams& P, LocalMapState& out) {
  for (int i = 0; i < 6; i++) out.cube[i] = in.cube[i];
  out.initialized = 1;
  out.n_boxes = 0;
  out.moves = in.moves;
  for (int i = 0; i < 18; i++) out.boxes[i] = 0.f;
  if (!in.initialized) {
    for (int i = 0; i < 3; i++) {
      out.cube[i] = (float)(pos[i] - P.cube_len / 2.0);
      out.cube[3 + i] = (float)(pos[i] + P.cube_len / 2.0);
    }
    return;
  }
  float d0[3], d1[3];
  if (!fov_need_move(in.cube, pos, P.thr, d0, d1)) return;
  for (int i = 0; i < 3; i++) {  // x, y, z; the low side before the high side
    float* b = out.boxes + 6 * out.n_boxes;
    if (d0[i] <= P.thr) {
      out.cube[3 + i] -= P.mov_dist;
      out.cube[i] -= P.mov_dist;
      for (int k = 0; k < 6; k++) b[k] = in.cube[k];
      b[i] = in.cube[3 + i] - P.mov_dist;
      out.n_boxes++;
    } else if (d1[i] <= P.thr) {
      out.cube[3 + i] += P.mov_dist;
      out.cube[i] += P.mov_dist;
      for (int k = 0; k < 6; k++) b[k] = in.cube[k];
      b[3 + i] = in.cube[i] + P.mov_dist;
      out.n_boxes++;
    }
  }
  out.moves = in.moves + 1;
}

}  // namespace lii
