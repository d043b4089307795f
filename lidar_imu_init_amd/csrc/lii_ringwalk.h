// The exact k-nearest search for an arbitrary point, ONE WAVEFRONT PER QUERY, as the units that search for points of their own share it:
// the map queries (lii_query.hip: lii_map_nearest, lii_map_radius) and the pose scoring (lii_score.hip).  The walk is described at the head
// of lii_query.hip.  Every loop is bounded by a number known before it starts; every table access is checked (cell_range_checked).
// Beside it the BALL walk (ball_walk): every point within max_d2, handed 64 at a time to a functor - the ball query lists them
// (lii_query.hip: k_map_radius), the surface statistics reduce them (lii_surface.hip: k_map_surface).
#pragma once
#include "lii_search.h"

namespace lii {

// d2 is a float32 sum of three rounded squares (relative error < 4e-7).  A geometric lower bound is compared with it only after
// it has been made smaller by eps on every axis (as axis_gap does) AND by this factor: a bound never prunes what d2 would accept.
constexpr float kBoundSlack = 0.99999f;
constexpr unsigned int kFree = 0xFFFFFFFFu;

// cell_range (lii_grid.h) with every bound checked: the probe ends after one trip round the table, an entry beyond the cell tables
// or a range beyond the point array reads as empty / is cut.  (The tables are consistent whenever this runs - the launch sits behind
// every update on the stream - so none of the checks fires; they are what "cannot read out of bounds for any input" rests on.)
__device__ __forceinline__ uint2 cell_range_checked(const GridView& g, unsigned int n_entries, unsigned int pts_cap, int ix, int iy, int iz) {
  const int bb = kCellBias >> kCoarseShift;
  const int bx = (ix >> kCoarseShift) + bb, by = (iy >> kCoarseShift) + bb, bz = (iz >> kCoarseShift) + bb;
  const unsigned long long bk = pack_block(bx, by, bz);
  unsigned int sl = hash_block(bx, by, bz) & g.block_mask;
  for (unsigned int probe = 0; probe <= g.block_mask; probe++) {
    const BlockEntry e = g.blocks[sl];
    if (e.key == bk) {
      const unsigned long long entry = (unsigned long long)e.id * kBlockCells + local_cell(ix, iy, iz);
      if (entry >= n_entries) break;
      uint2 r = g.cells[(size_t)entry];
      r.y = min(r.y, pts_cap);
      r.x = min(r.x, r.y);
      return r;
    }
    if (e.key == kEmptyKey) break;
    sl = (sl + 1) & g.block_mask;
  }
  return make_uint2(0u, 0u);
}

// Cell t of the Chebyshev ring r >= 1 around the origin, t < (2r + 1)^3 - (2r - 1)^3: the two z faces whole, the two y faces without
// the rows the z faces hold, the two x faces without both.
__device__ __forceinline__ void ring_cell(int r, int t, int& dx, int& dy, int& dz) {
  const int s = 2 * r + 1, m = s - 2;
  if (t < 2 * s * s) {
    const int f = t / (s * s), u = t - f * s * s;
    dz = f ? r : -r; dy = u / s - r; dx = u % s - r;
    return;
  }
  t -= 2 * s * s;
  if (t < 2 * s * m) {
    const int f = t / (s * m), u = t - f * s * m;
    dy = f ? r : -r; dz = u / s - (r - 1); dx = u % s - r;
    return;
  }
  t -= 2 * s * m;
  const int f = t / (m * m), u = t - f * m * m;
  dx = f ? r : -r; dz = u / m - (r - 1); dy = u % m - (r - 1);
}

// the query's cell on one axis, kept where r_max rings around it cannot overflow an int (a query that far out reaches no cell of the grid)
__device__ __forceinline__ int query_cell(float q, float inv_cs) {
  const float lim = (float)(2 * kCellBias);
  return (int)fminf(fmaxf(floorf(q * inv_cs), -lim), lim);
}

// The ball walk: EVERY live map point with d2 <= max_d2 around (qx, qy, qz), by the whole wavefront (every lane calls it with the same
// arguments), 64 points a trip: Chebyshev rings 0 .. r_max, one cell per lane, cell_range_checked, the per-cell gap bound against max_d2
// alone, the wave-wide prefix over 64 cells.  There is no k-th distance to stop on: ring r_max is always reached.  Per trip every lane
// calls trip(slot, have, in_ball, hits, mx, my, mz, d): its point's slot in the array, whether the trip has a point for it, whether
// that point is in the ball (float32 dist2_ref <= max_d2, inclusive), the ballot of in_ball over the wavefront, the point and its d2.
// What the caller does with a trip - list the points (k_map_radius), or reduce them (k_map_surface) - is the functor's business; the
// order of the trips and the lane a point falls to depend on the query and the map state alone.  wanted == false, a NaN coordinate or a
// ball that reaches no addressable cell: no trip.  Every loop is bounded by a number known before it starts.
template <class Trip>
__device__ __forceinline__ void ball_walk(const GridView& g, unsigned int n_entries, unsigned int pts_cap, float qx, float qy, float qz, float max_d2,
                                          int r_max, bool wanted, Trip&& trip) {
  const int lane = threadIdx.x & 63;
  const int cx = query_cell(qx, g.inv_cs), cy = query_cell(qy, g.inv_cs), cz = query_cell(qz, g.inv_cs);
  const float eps = 1e-6f * (fabsf(qx) + fabsf(qy) + fabsf(qz) + 8.f);
  const int reach = kCellBias + r_max;
  const bool searchable = wanted && qx == qx && qy == qy && qz == qz && abs(cx) <= reach && abs(cy) <= reach && abs(cz) <= reach;
  const int rings = searchable ? r_max : -1;
  for (int r = 0; r <= rings; r++) {
    const int s = 2 * r + 1;
    const int n_cells = r == 0 ? 1 : s * s * s - (s - 2) * (s - 2) * (s - 2);
    for (int t0 = 0; t0 < n_cells; t0 += 64) {
      const int t = t0 + lane;
      unsigned int first = 0u, cnt = 0u;
      if (t < n_cells) {
        int dx = 0, dy = 0, dz = 0;
        if (r > 0) ring_cell(r, t, dx, dy, dz);
        const int ix = cx + dx, iy = cy + dy, iz = cz + dz;
        // (a cell outside the addressable grid holds no map point: the ball's cell range is clamped to the grid)
        const bool in_grid = (unsigned)(ix + kCellBias) < 2u * kCellBias && (unsigned)(iy + kCellBias) < 2u * kCellBias && (unsigned)(iz + kCellBias) < 2u * kCellBias;
        if (in_grid) {
          const float gx = axis_gap(qx, ix, g.cs, eps), gy = axis_gap(qy, iy, g.cs, eps), gz = axis_gap(qz, iz, g.cs, eps);
          const float gap2 = (gx * gx + gy * gy + gz * gz) * kBoundSlack;
          if (!(gap2 > max_d2)) {
            const uint2 rg = cell_range_checked(g, n_entries, pts_cap, ix, iy, iz);
            first = rg.x;
            cnt = min(rg.y - rg.x, 1u << 25);  // (the point array holds fewer than 2^28 slots: the sum over 64 cells stays inside 32 bits whatever the tables say)
          }
        }
      }
      // the 64 ranges end to end: incl = points up to and including this lane's cell
      unsigned int incl = cnt;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
      }
      const unsigned int total = __shfl(incl, 63);
      const unsigned int cell_base = first - (incl - cnt);  // slot of point p of the sequence, p in this lane's cell: cell_base + p
      for (unsigned int p0 = 0; p0 < total; p0 += 64) {
        const unsigned int p = p0 + (unsigned)lane;
        const bool have = p < total;
        int j = 0;  // the first cell whose inclusive count exceeds p
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) {
          const unsigned int v = __shfl(incl, j + step - 1);
          if (v <= p) j += step;
        }
        const unsigned int slot = __shfl(cell_base, j) + p;
        float d = INFINITY, mx = 0.f, my = 0.f, mz = 0.f;
        if (have) {
          const F3 m = load_xyz(g.pts, slot);
          mx = m.x; my = m.y; mz = m.z;
          d = dist2_ref(qx, qy, qz, mx, my, mz);
        }
        const bool in_ball = have && d <= max_d2;
        const unsigned long long hits = __ballot(in_ball);
        trip(slot, have, in_ball, hits, mx, my, mz, d);
      }
    }
  }
}

// The k <= 64 nearest map points of (qx, qy, qz) with d2 <= max_d2, by the whole wavefront (every lane calls it with the same query):
// on return lane j holds entry j - (my_d, my_i = slot in the point array), ascending in d2; free entries: (+inf, kFree).  An equal d2
// stands BEHIND the entries found earlier, and a candidate equal to the k-th distance of a full list stays out.  A NaN coordinate, or a
// ball that reaches no addressable cell: no result.
__device__ __forceinline__ void ring_walk_nearest(const GridView& g, unsigned int n_entries, unsigned int pts_cap, float qx, float qy, float qz, int k,
                                                  float max_d2, int r_max, float& my_d, unsigned int& my_i) {
  const int lane = threadIdx.x & 63;
  my_d = INFINITY;
  my_i = kFree;
  const int cx = query_cell(qx, g.inv_cs), cy = query_cell(qy, g.inv_cs), cz = query_cell(qz, g.inv_cs);
  const float eps = 1e-6f * (fabsf(qx) + fabsf(qy) + fabsf(qz) + 8.f);
  // a NaN coordinate: no result; a ball that reaches no addressable cell (every cell visited is within r_max of the query's): none either
  const int reach = kCellBias + r_max;
  const bool searchable = qx == qx && qy == qy && qz == qz && abs(cx) <= reach && abs(cy) <= reach && abs(cz) <= reach;
  const int rings = searchable ? r_max : -1;
  for (int r = 0; r <= rings; r++) {
    const int s = 2 * r + 1;
    const int n_cells = r == 0 ? 1 : s * s * s - (s - 2) * (s - 2) * (s - 2);
    for (int t0 = 0; t0 < n_cells; t0 += 64) {
      const float kth0 = __shfl(my_d, k - 1);
      const int t = t0 + lane;
      unsigned int first = 0u, cnt = 0u;
      if (t < n_cells) {
        int dx = 0, dy = 0, dz = 0;
        if (r > 0) ring_cell(r, t, dx, dy, dz);
        const int ix = cx + dx, iy = cy + dy, iz = cz + dz;
        // (a cell outside the addressable grid holds no map point: the ball's cell range is clamped to the grid)
        const bool in_grid = (unsigned)(ix + kCellBias) < 2u * kCellBias && (unsigned)(iy + kCellBias) < 2u * kCellBias && (unsigned)(iz + kCellBias) < 2u * kCellBias;
        if (in_grid) {
          const float gx = axis_gap(qx, ix, g.cs, eps), gy = axis_gap(qy, iy, g.cs, eps), gz = axis_gap(qz, iz, g.cs, eps);
          const float gap2 = (gx * gx + gy * gy + gz * gz) * kBoundSlack;
          if (!(gap2 > fminf(max_d2, kth0))) {
            const uint2 rg = cell_range_checked(g, n_entries, pts_cap, ix, iy, iz);
            first = rg.x;
            cnt = min(rg.y - rg.x, 1u << 25);  // (the point array holds fewer than 2^28 slots: the sum over 64 cells stays inside 32 bits whatever the tables say)
          }
        }
      }
      // the 64 ranges end to end: incl = points up to and including this lane's cell
      unsigned int incl = cnt;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
      }
      const unsigned int total = __shfl(incl, 63);
      const unsigned int base = first - (incl - cnt);  // slot of point p of the sequence, p in this lane's cell: base + p
      for (unsigned int p0 = 0; p0 < total; p0 += 64) {
        const unsigned int p = p0 + (unsigned)lane;
        const bool have = p < total;
        int j = 0;  // the first cell whose inclusive count exceeds p
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) {
          const unsigned int v = __shfl(incl, j + step - 1);
          if (v <= p) j += step;
        }
        const unsigned int slot = __shfl(base, j) + p;
        float d = INFINITY;
        if (have) {
          const F3 m = load_xyz(g.pts, slot);
          d = dist2_ref(qx, qy, qz, m.x, m.y, m.z);
        }
        float kth = __shfl(my_d, k - 1);
        unsigned long long cand = __ballot(have && d <= max_d2 && d < kth);
        while (cand) {  // (at most 64 trips: every trip clears the lowest bit)
          const int src = __ffsll((long long)cand) - 1;
          const float cd = __shfl(d, src);
          const unsigned int ci = __shfl(slot, src);
          const int pos = __popcll(__ballot(my_d <= cd));  // behind every entry that is not larger; < k, because cd < kth
          const float up_d = __shfl_up(my_d, 1);
          const unsigned int up_i = __shfl_up(my_i, 1);
          if (lane > pos) { my_d = up_d; my_i = up_i; }
          else if (lane == pos) { my_d = cd; my_i = ci; }
          kth = __shfl(my_d, k - 1);
          cand &= cand - 1ull;
          cand &= __ballot(d < kth);
        }
      }
    }
    // what lies outside the visited cube [c - r, c + r]^3 is at least `bound` away (0 when the query is not inside its own cell's box)
    const float kth = __shfl(my_d, k - 1);
    const float bx = fminf(qx - (float)(cx - r) * g.cs, (float)(cx + r + 1) * g.cs - qx);
    const float by = fminf(qy - (float)(cy - r) * g.cs, (float)(cy + r + 1) * g.cs - qy);
    const float bz = fminf(qz - (float)(cz - r) * g.cs, (float)(cz + r + 1) * g.cs - qz);
    const float bound = fmaxf(fminf(fminf(bx, by), bz) - eps, 0.f);
    const float bd2 = bound * bound * kBoundSlack;
    if (kth < bd2 || max_d2 < bd2) break;
  }
}

}  // namespace lii
